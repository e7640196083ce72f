// Levelled max-min point ordering on the GPU (nngp_order_maxmin; the definition is in order_maxmin.h and
// DESIGN.md 4.4a).
//
// Per level two open-addressing hash tables keyed by the packed cell, rebuilt from empty: table A holds the points
// selected so far (they are pairwise >= r apart, two points of one cell are closer than r: at most one per cell),
// the winners' table holds, per non-empty cell of a round, the smallest key of U in it (64-bit atomicMin).  A
// point looks at the 5^D cells around its own for everything that can be closer than r.  The sequential visit of
// the winners runs as Luby rounds: a live winner with no live or accepted smaller-key winner closer than r is
// accepted, live winners closer than r to an accepted one retire; what this accepts is exactly the sequential
// set, whatever the scheduling.  Lists (the unselected, U, the selected) are appended through atomic counters, so
// their order varies from run to run; nothing reads that order: every decision is a minimum over keys or a set
// membership, and the output is sorted by (level, key).
//
// The host loop reads one 256-byte control block per round (the counts it sizes the next launches by).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "geom.h"
#include "nngp_internal.h"
#include "order_maxmin.h"

namespace nngp {

namespace {

using u64 = unsigned long long;
constexpr u64 kEmpty = ~0ull;
constexpr int32_t kLive = 1, kAccepted = 2, kRetired = 3;

struct MmCtl {  // device control block (256 B): reductions of the start, counters of the rounds
    u64 d2min_bits;    // min dist2(x_i, centre) as ordered bits
    u64 r2max_bits;    // max dist2(x_i, p1) as ordered bits
    uint32_t p1;
    uint32_t err;      // a probe sequence ran through a whole table
    uint32_t n_rem;    // unselected points kept for the next level
    uint32_t n_u;      // |U| after marking / after a round
    uint32_t n_w;      // winners of the round
    uint32_t n_live;   // live winners after a Luby iteration
    uint32_t n_new;    // points the round selected
    uint32_t pad;
    Bbox box;
    char fill[256 - 2 * 8 - 8 * 4 - sizeof(Bbox)];
};
static_assert(sizeof(MmCtl) == 256, "MmCtl is one 256-byte block");

struct MmLevel {
    double lo[kMaxDim];
    double h, r2;
    int32_t level;
};

struct MmTable {
    u64* key;      // packed cell, kEmpty when free
    u64 mask;      // capacity - 1
};

// ((d0 d0) + (d1 d1)) + (d2 d2), every operation rounded on its own (hipcc contracts a * b + c by default)
template <int D>
__device__ __forceinline__ double dist2(const double (&a)[D], const double (&b)[D]) {
#pragma clang fp contract(off)
    const double t0 = a[0] - b[0];
    double d = t0 * t0;
#pragma unroll
    for (int k = 1; k < D; ++k) {
        const double t = a[k] - b[k];
        const double q = t * t;
        d = d + q;
    }
    return d;
}

template <int D>
__device__ __forceinline__ void cell_of(const double (&x)[D], const MmLevel& L, int64_t (&c)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) c[k] = (int64_t)floor((x[k] - L.lo[k]) / L.h);
}

template <int D>
__device__ __forceinline__ u64 pack_cell(const int64_t (&c)[D]) {
    u64 p = (u64)c[0];
    if constexpr (D > 1) p |= (u64)c[1] << 21;
    if constexpr (D > 2) p |= (u64)c[2] << 42;
    return p;
}

__device__ __forceinline__ u64 hash_cell(u64 x) {  // the murmur3 64-bit finaliser
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// slot of `cell`, or -1 when the table does not hold it (the probe ends at the first free slot; a table is never
// more than half full, and the loop is bounded by the capacity whatever it holds)
__device__ __forceinline__ int64_t find_slot(const MmTable& T, u64 cell) {
    u64 s = hash_cell(cell) & T.mask;
    for (u64 probe = 0; probe <= T.mask; ++probe) {
        const u64 k = T.key[s];
        if (k == cell) return (int64_t)s;
        if (k == kEmpty) return -1;
        s = (s + 1) & T.mask;
    }
    return -1;
}

// slot of `cell`, claimed if the table did not hold it; -1 (and ctl->err) when the whole table was probed
__device__ __forceinline__ int64_t claim_slot(const MmTable& T, u64 cell, MmCtl* ctl) {
    u64 s = hash_cell(cell) & T.mask;
    for (u64 probe = 0; probe <= T.mask; ++probe) {
        u64 k = T.key[s];
        if (k == kEmpty) k = atomicCAS(&T.key[s], kEmpty, cell);
        if (k == kEmpty || k == cell) return (int64_t)s;
        s = (s + 1) & T.mask;
    }
    ctl->err = 1u;
    return -1;
}

// f(slot) for every occupied slot among the 5^D cells around c (cells below 0 do not exist)
template <int D, typename F>
__device__ __forceinline__ void for_near_slots(const MmTable& T, const int64_t (&c)[D], F f) {
    constexpr int kCells = D == 1 ? 5 : (D == 2 ? 25 : 125);
    for (int t = 0; t < kCells; ++t) {
        int64_t nc[D];
        int rest = t;
        bool inside = true;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            nc[k] = c[k] + (rest % 5) - 2;
            rest /= 5;
            inside = inside && nc[k] >= 0;
        }
        if (!inside) continue;
        const int64_t s = find_slot(T, pack_cell<D>(nc));
        if (s >= 0) f(s);
    }
}

__device__ __forceinline__ u64 key_of(uint32_t i, uint32_t seed) {
    uint32_t h = i + seed * 0x9e3779b9u;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return ((u64)h << 32) | i;
}

__device__ __forceinline__ int64_t gtid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }

// ---------------------------------------------------------------- the start: p1 and R
__global__ __launch_bounds__(256) void mm_init(int64_t n, int32_t* __restrict__ level, int32_t* __restrict__ rem,
                                               MmCtl* __restrict__ ctl) {
    for (int64_t i = gtid(); i < n; i += gstride()) {
        level[i] = kMaxminTail;
        rem[i] = (int32_t)i;
    }
    if (gtid() == 0) {
        ctl->d2min_bits = kEmpty;
        ctl->r2max_bits = 0ull;
        ctl->p1 = 0xffffffffu;
        ctl->err = 0u;
    }
}

template <int D>
__device__ __forceinline__ void centre_of(const Bbox& b, double (&c)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) c[k] = 0.5 * (b.lo[k] + b.hi[k]);
}

// dist2 is >= 0 (or NaN), so its bits order as unsigned integers; a NaN is above every number
template <int D>
__global__ __launch_bounds__(256) void mm_centre_min(const double* __restrict__ p, int64_t n, MmCtl* __restrict__ ctl) {
    double c[D];
    centre_of<D>(ctl->box, c);
    u64 best = kEmpty;
    for (int64_t i = gtid(); i < n; i += gstride()) {
        double x[D];
        load_point<D>(p + i * D, x);
        const u64 b = (u64)__double_as_longlong(dist2<D>(x, c));
        best = b < best ? b : best;
    }
    if (best != kEmpty) atomicMin(&ctl->d2min_bits, best);
}

template <int D>
__global__ __launch_bounds__(256) void mm_centre_arg(const double* __restrict__ p, int64_t n, MmCtl* __restrict__ ctl) {
    double c[D];
    centre_of<D>(ctl->box, c);
    const u64 want = ctl->d2min_bits;
    uint32_t best = 0xffffffffu;
    for (int64_t i = gtid(); i < n; i += gstride()) {
        double x[D];
        load_point<D>(p + i * D, x);
        if ((u64)__double_as_longlong(dist2<D>(x, c)) == want && (uint32_t)i < best) best = (uint32_t)i;
    }
    if (best != 0xffffffffu) atomicMin(&ctl->p1, best);
}

template <int D>
__global__ __launch_bounds__(256) void mm_radius(const double* __restrict__ p, int64_t n, int32_t* __restrict__ level,
                                                 int32_t* __restrict__ sel, MmCtl* __restrict__ ctl) {
    const uint32_t p1 = ctl->p1;
    if (p1 >= (uint32_t)n) return;  // no point matched the minimum (a NaN coordinate): the host refuses
    double o[D];
    load_point<D>(p + (int64_t)p1 * D, o);
    u64 best = 0ull;
    for (int64_t i = gtid(); i < n; i += gstride()) {
        double x[D];
        load_point<D>(p + i * D, x);
        const u64 b = (u64)__double_as_longlong(dist2<D>(x, o));
        best = b > best ? b : best;
    }
    atomicMax(&ctl->r2max_bits, best);
    if (gtid() == 0) {
        level[p1] = 0;
        sel[0] = (int32_t)p1;
    }
}

// ---------------------------------------------------------------- a level
// table A: the cell of every selected point -> the point
template <int D>
__global__ __launch_bounds__(256) void mm_build_a(const double* __restrict__ p, const int32_t* __restrict__ sel,
                                                  int64_t n_sel, MmLevel L, MmTable A, int32_t* __restrict__ a_val,
                                                  MmCtl* __restrict__ ctl) {
    for (int64_t j = gtid(); j < n_sel; j += gstride()) {
        const int32_t i = sel[j];
        double x[D];
        load_point<D>(p + (int64_t)i * D, x);
        int64_t c[D];
        cell_of<D>(x, L, c);
        const int64_t s = claim_slot(A, pack_cell<D>(c), ctl);
        if (s >= 0) a_val[s] = i;
    }
}

// the unselected points of rem_in go to rem_out, and to U when no point of A is closer than r
template <int D>
__global__ __launch_bounds__(256) void mm_mark(const double* __restrict__ p, const int32_t* __restrict__ rem_in,
                                               int64_t n_rem, const int32_t* __restrict__ level, MmLevel L, MmTable A,
                                               const int32_t* __restrict__ a_val, int32_t* __restrict__ rem_out,
                                               int32_t* __restrict__ u_out, MmCtl* __restrict__ ctl) {
    for (int64_t j = gtid(); j < n_rem; j += gstride()) {
        const int32_t i = rem_in[j];
        if (level[i] != kMaxminTail) continue;
        rem_out[atomicAdd(&ctl->n_rem, 1u)] = i;
        double x[D];
        load_point<D>(p + (int64_t)i * D, x);
        int64_t c[D];
        cell_of<D>(x, L, c);
        bool far = true;
        for_near_slots<D>(A, c, [&](int64_t s) {
            double y[D];
            load_point<D>(p + (int64_t)a_val[s] * D, y);
            far = far && dist2<D>(x, y) >= L.r2;
        });
        if (far) u_out[atomicAdd(&ctl->n_u, 1u)] = i;
    }
}

// winners' table: per cell the smallest key of U
template <int D>
__global__ __launch_bounds__(256) void mm_elect(const double* __restrict__ p, const int32_t* __restrict__ u,
                                                int64_t n_u, MmLevel L, MmTable W, u64* __restrict__ w_key,
                                                uint32_t seed, MmCtl* __restrict__ ctl) {
    for (int64_t j = gtid(); j < n_u; j += gstride()) {
        const int32_t i = u[j];
        double x[D];
        load_point<D>(p + (int64_t)i * D, x);
        int64_t c[D];
        cell_of<D>(x, L, c);
        const int64_t s = claim_slot(W, pack_cell<D>(c), ctl);
        if (s >= 0) atomicMin(&w_key[s], key_of((uint32_t)i, seed));
    }
}

// the winners become live and are listed by slot
template <int D>
__global__ __launch_bounds__(256) void mm_pick(const double* __restrict__ p, const int32_t* __restrict__ u,
                                               int64_t n_u, MmLevel L, MmTable W, const u64* __restrict__ w_key,
                                               int32_t* __restrict__ w_state, int32_t* __restrict__ w_list,
                                               uint32_t seed, MmCtl* __restrict__ ctl) {
    for (int64_t j = gtid(); j < n_u; j += gstride()) {
        const int32_t i = u[j];
        double x[D];
        load_point<D>(p + (int64_t)i * D, x);
        int64_t c[D];
        cell_of<D>(x, L, c);
        const int64_t s = find_slot(W, pack_cell<D>(c));
        if (s >= 0 && w_key[s] == key_of((uint32_t)i, seed)) {
            w_state[s] = kLive;
            w_list[atomicAdd(&ctl->n_w, 1u)] = (int32_t)s;
        }
    }
}

// Luby iteration, first half: a live winner is accepted unless a winner that is not retired, has a smaller key and
// is closer than r exists.  (Winners accepted in earlier iterations have retired every live winner within r, so an
// accepted one met here was accepted in this launch: it blocks exactly as it did while live.)
template <int D>
__global__ __launch_bounds__(256) void mm_accept(const double* __restrict__ p, MmLevel L, MmTable W,
                                                 const u64* __restrict__ w_key, int32_t* __restrict__ w_state,
                                                 const int32_t* __restrict__ w_list, const MmCtl* __restrict__ ctl) {
    const int64_t n_w = ctl->n_w;
    for (int64_t j = gtid(); j < n_w; j += gstride()) {
        const int64_t s = w_list[j];
        if (w_state[s] != kLive) continue;
        const u64 mine = w_key[s];
        double x[D];
        load_point<D>(p + (int64_t)(uint32_t)mine * D, x);
        int64_t c[D];
        cell_of<D>(x, L, c);
        bool blocked = false;
        for_near_slots<D>(W, c, [&](int64_t t) {
            const u64 other = w_key[t];
            if (t == s || other >= mine || w_state[t] == kRetired) return;
            double y[D];
            load_point<D>(p + (int64_t)(uint32_t)other * D, y);
            blocked = blocked || dist2<D>(x, y) < L.r2;
        });
        if (!blocked) w_state[s] = kAccepted;
    }
}

// second half: a live winner closer than r to an accepted one retires; the rest are counted
template <int D>
__global__ __launch_bounds__(256) void mm_retire(const double* __restrict__ p, MmLevel L, MmTable W,
                                                 const u64* __restrict__ w_key, int32_t* __restrict__ w_state,
                                                 const int32_t* __restrict__ w_list, MmCtl* __restrict__ ctl) {
    const int64_t n_w = ctl->n_w;
    for (int64_t j = gtid(); j < n_w; j += gstride()) {
        const int64_t s = w_list[j];
        if (w_state[s] != kLive) continue;
        double x[D];
        load_point<D>(p + (int64_t)(uint32_t)w_key[s] * D, x);
        int64_t c[D];
        cell_of<D>(x, L, c);
        bool out = false;
        for_near_slots<D>(W, c, [&](int64_t t) {
            if (w_state[t] != kAccepted) return;
            double y[D];
            load_point<D>(p + (int64_t)(uint32_t)w_key[t] * D, y);
            out = out || dist2<D>(x, y) < L.r2;
        });
        if (out) w_state[s] = kRetired;
        else atomicAdd(&ctl->n_live, 1u);
    }
}

// end of a round: the accepted winners are selected; every point of U closer than r to one leaves U
template <int D>
__global__ __launch_bounds__(256) void mm_remove(const double* __restrict__ p, const int32_t* __restrict__ u,
                                                 int64_t n_u, MmLevel L, MmTable W, const u64* __restrict__ w_key,
                                                 const int32_t* __restrict__ w_state, int32_t* __restrict__ level,
                                                 int32_t* __restrict__ sel, int64_t n_sel, int64_t n,
                                                 int32_t* __restrict__ u_out, MmCtl* __restrict__ ctl) {
    for (int64_t j = gtid(); j < n_u; j += gstride()) {
        const int32_t i = u[j];
        double x[D];
        load_point<D>(p + (int64_t)i * D, x);
        int64_t c[D];
        cell_of<D>(x, L, c);
        bool gone = false, chosen = false;
        for_near_slots<D>(W, c, [&](int64_t t) {
            if (w_state[t] != kAccepted) return;
            const uint32_t v = (uint32_t)w_key[t];
            if (v == (uint32_t)i) {
                chosen = gone = true;
                return;
            }
            double y[D];
            load_point<D>(p + (int64_t)v * D, y);
            gone = gone || dist2<D>(x, y) < L.r2;
        });
        if (chosen) {
            const int64_t at = n_sel + (int64_t)atomicAdd(&ctl->n_new, 1u);
            level[i] = L.level;
            if (at < n) sel[at] = i;  // a point is chosen once, so at < n; the guard keeps a fault out of reach
        } else if (!gone) {
            u_out[atomicAdd(&ctl->n_u, 1u)] = i;
        }
    }
}

// ---------------------------------------------------------------- the output: sorted by (level, hash, index)
__global__ __launch_bounds__(256) void mm_sort_keys(int64_t n, const int32_t* __restrict__ level, uint32_t seed,
                                                    u64* __restrict__ key, int32_t* __restrict__ val) {
    for (int64_t i = gtid(); i < n; i += gstride()) {
        key[i] = ((u64)(uint32_t)level[i] << 32) | (key_of((uint32_t)i, seed) >> 32);
        val[i] = (int32_t)i;
    }
}

__global__ __launch_bounds__(256) void mm_emit(int64_t n, const u64* __restrict__ key, const int32_t* __restrict__ val,
                                               int64_t* __restrict__ perm, int32_t* __restrict__ level) {
    for (int64_t i = gtid(); i < n; i += gstride()) {
        perm[i] = (int64_t)val[i];
        level[i] = (int32_t)(key[i] >> 32);
    }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

constexpr int kSortBits = 37;  // 32 bits of hash under 5 bits of level

size_t sort_temp_bytes(int64_t n) {
    size_t tb = 0;
    if (rocprim::radix_sort_pairs((void*)nullptr, tb, (const u64*)nullptr, (u64*)nullptr, (const int32_t*)nullptr,
                                  (int32_t*)nullptr, (size_t)n, 0u, (unsigned)kSortBits) != hipSuccess)
        return 0;
    return tb < 256 ? 256 : tb;
}

struct MmLayout {
    size_t stats, ctl, part, level, rem[2], u[2], sel, w_list, a_key, a_val, w_cell, w_key, w_state, sort_key[2],
        sort_val[2], sort_tmp, total;
    uint64_t cap_max;
};

bool layout(int64_t n, MmLayout* o) {
    const size_t tb = sort_temp_bytes(n);
    if (tb == 0) return false;
    o->cap_max = maxmin_table_capacity((uint64_t)n);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += align256(bytes);
        return here;
    };
    const size_t n4 = (size_t)n * 4, n8 = (size_t)n * 8, c4 = (size_t)o->cap_max * 4, c8 = (size_t)o->cap_max * 8;
    o->stats = take(sizeof(MaxminStats));
    o->ctl = take(sizeof(MmCtl));
    o->part = take(2 * kMaxDim * 256 * sizeof(double));
    o->level = take(n4);
    o->rem[0] = take(n4);
    o->rem[1] = take(n4);
    o->u[0] = take(n4);
    o->u[1] = take(n4);
    o->sel = take(n4);
    o->w_list = take(n4);
    o->a_key = take(c8);
    o->a_val = take(c4);
    o->w_cell = take(c8);
    o->w_key = take(c8);  // directly behind w_cell: one fill clears both
    o->w_state = take(c4);
    o->sort_key[0] = take(n8);
    o->sort_key[1] = take(n8);
    o->sort_val[0] = take(n4);
    o->sort_val[1] = take(n4);
    o->sort_tmp = take(tb);
    o->total = at;
    return true;
}

unsigned blocks_for(int64_t work) {
    const int64_t b = (work + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

template <int D>
MaxminStatus run(const double* coords, int64_t n, uint32_t seed, int64_t* perm_out, int32_t* level_out, char* ws,
                 const MmLayout& lay, hipStream_t s, hipError_t* err) {
    MaxminStats st;
    memset(&st, 0, sizeof st);
    MmCtl* ctl = (MmCtl*)(ws + lay.ctl);
    double* part = (double*)(ws + lay.part);
    int32_t* level = (int32_t*)(ws + lay.level);
    int32_t* rem[2] = {(int32_t*)(ws + lay.rem[0]), (int32_t*)(ws + lay.rem[1])};
    int32_t* u[2] = {(int32_t*)(ws + lay.u[0]), (int32_t*)(ws + lay.u[1])};
    int32_t* sel = (int32_t*)(ws + lay.sel);
    int32_t* w_list = (int32_t*)(ws + lay.w_list);
    u64* a_key = (u64*)(ws + lay.a_key);
    int32_t* a_val = (int32_t*)(ws + lay.a_val);
    u64* w_cell = (u64*)(ws + lay.w_cell);
    int32_t* w_state = (int32_t*)(ws + lay.w_state);
    const dim3 T(256);
    MmCtl h;

#define MM_TRY(call)                           \
    do {                                       \
        if ((*err = (call)) != hipSuccess) return kMaxminHipError; \
    } while (0)
#define MM_LAUNCHED()   \
    do {                \
        ++st.launches;  \
        MM_TRY(hipGetLastError()); \
    } while (0)
    auto read_ctl = [&]() -> hipError_t {
        ++st.host_reads;
        hipError_t e = hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    };
    // the counters n_rem .. pad, zeroed before the launches that count into them
    auto zero_counts = [&]() -> hipError_t {
        ++st.launches;
        return hipMemsetAsync(&ctl->n_rem, 0, 6 * sizeof(uint32_t), s);
    };

    // the start: bounding box, p1, R
    hipLaunchKernelGGL(mm_init, dim3(blocks_for(n)), T, 0, s, n, level, rem[0], ctl);
    MM_LAUNCHED();
    hipLaunchKernelGGL((bbox_partial<D>), dim3(256), T, 0, s, coords, n, part);
    MM_LAUNCHED();
    hipLaunchKernelGGL((bbox_final<D>), dim3(1), dim3(64), 0, s, (const double*)part, 256, &ctl->box);
    MM_LAUNCHED();
    hipLaunchKernelGGL((mm_centre_min<D>), dim3(blocks_for(n)), T, 0, s, coords, n, ctl);
    MM_LAUNCHED();
    hipLaunchKernelGGL((mm_centre_arg<D>), dim3(blocks_for(n)), T, 0, s, coords, n, ctl);
    MM_LAUNCHED();
    hipLaunchKernelGGL((mm_radius<D>), dim3(blocks_for(n)), T, 0, s, coords, n, level, sel, ctl);
    MM_LAUNCHED();
    MM_TRY(read_ctl());
    double R2;
    memcpy(&R2, &h.r2max_bits, sizeof R2);
    if (h.p1 >= (uint32_t)n || !isfinite(R2)) return kMaxminNotFinite;
    for (int k = 0; k < D; ++k)
        if (!isfinite(h.box.lo[k]) || !isfinite(h.box.hi[k])) return kMaxminNotFinite;
    const double R = sqrt(R2);
    st.selected[0] = 1;

    int64_t n_sel = 1, n_rem = n;
    int cur_rem = 0;
    for (int l = 1; l <= kMaxminLevels && n_sel < n; ++l) {
        MaxminLevel lv;
        if (!maxmin_level(R, D, l, &lv)) break;
        st.levels = l;
        MmLevel L;
        for (int k = 0; k < kMaxDim; ++k) L.lo[k] = k < D ? h.box.lo[k] : 0.0;
        L.h = lv.h;
        L.r2 = lv.r2;
        L.level = l;
        const uint64_t cells = maxmin_cell_bound(h.box.lo, h.box.hi, D, lv.h, (uint64_t)n);

        const MmTable A{a_key, maxmin_table_capacity((uint64_t)n_sel) - 1};
        MM_TRY(hipMemsetAsync(a_key, 0xff, (size_t)(A.mask + 1) * 8, s));
        ++st.launches;
        hipLaunchKernelGGL((mm_build_a<D>), dim3(blocks_for(n_sel)), T, 0, s, coords, (const int32_t*)sel, n_sel, L, A,
                           a_val, ctl);
        MM_LAUNCHED();
        MM_TRY(zero_counts());
        hipLaunchKernelGGL((mm_mark<D>), dim3(blocks_for(n_rem)), T, 0, s, coords, (const int32_t*)rem[cur_rem], n_rem,
                           (const int32_t*)level, L, A, (const int32_t*)a_val, rem[cur_rem ^ 1], u[0], ctl);
        MM_LAUNCHED();
        MM_TRY(read_ctl());
        if (h.err) return kMaxminTableOverflow;
        cur_rem ^= 1;
        n_rem = h.n_rem;
        int64_t n_u = h.n_u;
        int cur_u = 0;
        while (n_u > 0) {
            ++st.rounds[l];
            const uint64_t bound = (uint64_t)n_u < cells ? (uint64_t)n_u : cells;
            const uint64_t cap = maxmin_table_capacity(bound);
            const MmTable W{w_cell, cap - 1};
            u64* w_key = w_cell + cap;  // inside [w_cell, w_cell + 2 cap_max)
            MM_TRY(hipMemsetAsync(w_cell, 0xff, (size_t)cap * 16, s));
            ++st.launches;
            MM_TRY(zero_counts());
            hipLaunchKernelGGL((mm_elect<D>), dim3(blocks_for(n_u)), T, 0, s, coords, (const int32_t*)u[cur_u], n_u, L,
                               W, w_key, seed, ctl);
            MM_LAUNCHED();
            hipLaunchKernelGGL((mm_pick<D>), dim3(blocks_for(n_u)), T, 0, s, coords, (const int32_t*)u[cur_u], n_u, L, W,
                               (const u64*)w_key, w_state, w_list, seed, ctl);
            MM_LAUNCHED();
            const unsigned wb = blocks_for((int64_t)bound);  // the winners are at most `bound`
            uint32_t live_before = 0xffffffffu;
            for (bool first = true;; first = false) {
                ++st.luby[l];
                if (!first) {  // (zero_counts cleared it for the round's first iteration)
                    MM_TRY(hipMemsetAsync(&ctl->n_live, 0, sizeof(uint32_t), s));
                    ++st.launches;
                }
                hipLaunchKernelGGL((mm_accept<D>), dim3(wb), T, 0, s, coords, L, W, (const u64*)w_key, w_state,
                                   (const int32_t*)w_list, (const MmCtl*)ctl);
                MM_LAUNCHED();
                hipLaunchKernelGGL((mm_retire<D>), dim3(wb), T, 0, s, coords, L, W, (const u64*)w_key, w_state,
                                   (const int32_t*)w_list, ctl);
                MM_LAUNCHED();
                MM_TRY(read_ctl());
                if (h.err) return kMaxminTableOverflow;
                if (h.n_live == 0) break;
                // the live winner with the smallest key is always accepted, so the count falls: not reached
                if (h.n_live >= live_before) return kMaxminTableOverflow;
                live_before = h.n_live;
            }
            hipLaunchKernelGGL((mm_remove<D>), dim3(blocks_for(n_u)), T, 0, s, coords, (const int32_t*)u[cur_u], n_u, L,
                               W, (const u64*)w_key, (const int32_t*)w_state, level, sel, n_sel, n, u[cur_u ^ 1], ctl);
            MM_LAUNCHED();
            MM_TRY(read_ctl());
            cur_u ^= 1;
            n_u = h.n_u;
            n_sel += h.n_new;
            st.selected[l] += (int32_t)h.n_new;
            if (h.n_new == 0 || n_sel > n) return kMaxminTableOverflow;  // a round always selects: not reached
        }
    }
    st.n_tail = (int32_t)(n - n_sel);

    u64* key_in = (u64*)(ws + lay.sort_key[0]);
    u64* key_out = (u64*)(ws + lay.sort_key[1]);
    int32_t* val_in = (int32_t*)(ws + lay.sort_val[0]);
    int32_t* val_out = (int32_t*)(ws + lay.sort_val[1]);
    hipLaunchKernelGGL(mm_sort_keys, dim3(blocks_for(n)), T, 0, s, n, (const int32_t*)level, seed, key_in, val_in);
    MM_LAUNCHED();
    size_t tb = sort_temp_bytes(n);
    MM_TRY(rocprim::radix_sort_pairs((void*)(ws + lay.sort_tmp), tb, (const u64*)key_in, key_out,
                                     (const int32_t*)val_in, val_out, (size_t)n, 0u, (unsigned)kSortBits, s));
    ++st.launches;
    hipLaunchKernelGGL(mm_emit, dim3(blocks_for(n)), T, 0, s, n, (const u64*)key_out, (const int32_t*)val_out, perm_out,
                       level_out);
    MM_LAUNCHED();
    ++st.launches;
    MM_TRY(hipMemcpyAsync(ws + lay.stats, &st, sizeof st, hipMemcpyHostToDevice, s));
    MM_TRY(hipStreamSynchronize(s));  // st is on this frame
    return kMaxminOk;
#undef MM_TRY
#undef MM_LAUNCHED
}

}  // namespace

size_t order_maxmin_workspace_bytes(int64_t n, int dim) {
    if (n < 1 || n > INT32_MAX || dim < 1 || dim > kMaxDim) return 0;
    MmLayout lay;
    return layout(n, &lay) ? lay.total : 0;
}

MaxminStatus order_maxmin_launch(const double* coords, int64_t n, int dim, uint32_t seed, int64_t* perm_out,
                                 int32_t* level_out, void* workspace, hipStream_t s, hipError_t* err) {
    *err = hipSuccess;
    MmLayout lay;
    if (!layout(n, &lay)) {
        *err = hipErrorInvalidValue;
        return kMaxminHipError;
    }
    char* ws = (char*)workspace;
    switch (dim) {
        case 1: return run<1>(coords, n, seed, perm_out, level_out, ws, lay, s, err);
        case 2: return run<2>(coords, n, seed, perm_out, level_out, ws, lay, s, err);
        case 3: return run<3>(coords, n, seed, perm_out, level_out, ws, lay, s, err);
    }
    *err = hipErrorInvalidValue;
    return kMaxminHipError;
}

}  // namespace nngp
