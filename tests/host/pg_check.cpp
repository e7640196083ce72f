// CPU check of pynngp_amd/csrc/polya_gamma.h (the source the GPU kernels run): sample moments per (b, c)
// cell, edge cases and loop-round counters, printed as "key value" pairs for tests/test_pg_host.py.
// Usage: pg_check [log2 N]   (default 18: N = 2^18 draws per cell)
#define NNGP_PG_COUNT
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../pynngp_amd/csrc/polya_gamma.h"

using nngp::PgStream;

struct Counters {
    int max_prop = 0, max_ig = 0, max_series = 0;
    long long bad = 0, blocks = 0;
    void take(const PgStream& s, bool bad_) {
        if (s.max_prop > max_prop) max_prop = s.max_prop;
        if (s.max_ig > max_ig) max_ig = s.max_ig;
        if (s.max_series > max_series) max_series = s.max_series;
        bad += bad_;
        blocks += s.blocks;
    }
    void merge(const Counters& o) {
        if (o.max_prop > max_prop) max_prop = o.max_prop;
        if (o.max_ig > max_ig) max_ig = o.max_ig;
        if (o.max_series > max_series) max_series = o.max_series;
        bad += o.bad;
        blocks += o.blocks;
    }
};

static double draw(int32_t b, double c, uint64_t seed, uint64_t loc, uint64_t it, Counters* cn, bool* bad_out = nullptr) {
    PgStream s = nngp::pg_stream(seed, loc, it);
    bool bad = false;
    const double v = nngp::pg_draw(b, c, s, &bad);
    if (cn) cn->take(s, bad);
    if (bad_out) *bad_out = bad;
    return v;
}

static uint64_t bits(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

int main(int argc, char** argv) {
    const int lg = argc > 1 ? atoi(argv[1]) : 18;
    const int64_t N = (int64_t)1 << lg;
    const uint64_t seed = 20240611u;
    const int bs[] = {1, 2, 7, 64};
    const double cs[] = {0.0, 0.1, 1.0, 2.5, 10.0, 50.0, 1000.0};
    unsigned T = std::thread::hardware_concurrency();
    T = T < 1 ? 1 : (T > 16 ? 16 : T);
    Counters all;
    std::vector<double> x((size_t)N);
    int cell = 0;
    for (int b : bs)
        for (double c : cs) {
            std::vector<Counters> cn(T);
            std::vector<std::thread> th;
            const uint64_t it = 1 + (uint64_t)cell;
            for (unsigned t = 0; t < T; ++t)
                th.emplace_back([&, t] {
                    for (int64_t i = N * t / T; i < N * (t + 1) / T; ++i)
                        x[(size_t)i] = draw(b, c, seed, (uint64_t)i, it, &cn[t]);
                });
            for (auto& h : th) h.join();
            Counters cc;
            for (auto& k : cn) cc.merge(k);
            all.merge(cc);
            // fixed-order moments
            long double s1 = 0, sl = 0;
            double mn = INFINITY;
            int ok = 1;
            for (int64_t i = 0; i < N; ++i) {
                const double v = x[(size_t)i];
                if (!(v > 0.0) || !std::isfinite(v)) ok = 0;
                if (v < mn) mn = v;
                s1 += v;
                sl += std::exp(-v);
            }
            const long double mean = s1 / N;
            long double m2 = 0, m4 = 0;
            for (int64_t i = 0; i < N; ++i) {
                const long double d = x[(size_t)i] - mean;
                m2 += d * d;
                m4 += d * d * d * d;
            }
            printf("cell%d_b %d\ncell%d_c %.17g\n", cell, b, cell, c);
            printf("cell%d_mean %.17Lg\ncell%d_var %.17Lg\ncell%d_m4 %.17Lg\ncell%d_lap %.17Lg\n", cell, mean, cell,
                   m2 / (N - 1), cell, m4 / N, cell, sl / N);
            printf("cell%d_ok %d\ncell%d_min %.17g\ncell%d_bad %lld\ncell%d_max_prop %d\n", cell, ok, cell, mn, cell,
                   cc.bad, cell, cc.max_prop);
            ++cell;
        }
    printf("cells %d\nN %lld\n", cell, (long long)N);
    printf("max_prop %d\nmax_ig %d\nmax_series %d\ncap_hits %lld\nblocks %lld\n", all.max_prop, all.max_ig,
           all.max_series, all.bad, all.blocks);

    // b = 0: exactly 0.0, no block drawn, whatever c
    {
        Counters k;
        int ok = 1;
        for (double c : {0.0, 3.0, -1000.0, (double)NAN}) {
            const double v = draw(0, c, seed, 5, 9, &k);
            if (bits(v) != 0) ok = 0;
        }
        printf("b0_zero %d\nb0_blocks %lld\nb0_bad %lld\n", ok, k.blocks, k.bad);
    }
    // c and -c: identical bits
    {
        int ok = 1;
        for (double c : {0.1, 1.0, 2.5, 10.0, 50.0, 1000.0})
            for (int b : {1, 7})
                for (uint64_t i = 0; i < 2048; ++i)
                    if (bits(draw(b, c, seed, i, 3, nullptr)) != bits(draw(b, -c, seed, i, 3, nullptr))) ok = 0;
        printf("sign_symmetric %d\n", ok);
    }
    // position only: the draw does not depend on anything but (seed, iteration, location, b, c); other seeds /
    // iterations give other draws
    {
        const double a = draw(3, 1.5, seed, 77, 4, nullptr);
        printf("repeatable %d\n", bits(a) == bits(draw(3, 1.5, seed, 77, 4, nullptr)));
        printf("seed_changes %d\n", bits(a) != bits(draw(3, 1.5, seed + 1, 77, 4, nullptr)));
        printf("iteration_changes %d\n", bits(a) != bits(draw(3, 1.5, seed, 77, 5, nullptr)));
        printf("location_changes %d\n", bits(a) != bits(draw(3, 1.5, seed, 78, 4, nullptr)));
    }
    // non-finite c, bad b: NaN, flagged, before any loop (no block drawn)
    {
        Counters k;
        int ok = 1;
        bool bad;
        for (double c : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
            const double v = draw(3, c, seed, 1, 1, &k, &bad);
            if (!std::isnan(v) || !bad) ok = 0;
        }
        for (int b : {-1, NNGP_PG_MAX_TRIALS + 1, INT32_MIN, INT32_MAX}) {
            const double v = draw(b, 0.5, seed, 1, 1, &k, &bad);
            if (!std::isnan(v) || !bad) ok = 0;
        }
        printf("nonfinite_flagged %d\nnonfinite_blocks %lld\nnonfinite_rounds %d\n", ok, k.blocks,
               k.max_prop + k.max_ig + k.max_series);
    }
    // the largest b: finite, positive, near its mean b / 4 at c = 0
    {
        bool bad;
        const double v = draw(NNGP_PG_MAX_TRIALS, 0.0, seed, 11, 2, nullptr, &bad);
        printf("bmax_ok %d\n", !bad && std::isfinite(v) && v > 200.0 && v < 320.0);
    }
    // |c| <= 1000 sweep: finite and positive everywhere
    {
        int ok = 1;
        Counters k;
        for (int q = 0; q <= 4000; ++q) {
            const double c = 0.25 * q;
            for (uint64_t i = 0; i < 8; ++i) {
                const double v = draw(1, c, seed, i, 100 + q, &k);
                if (!(v > 0.0) || !std::isfinite(v)) ok = 0;
            }
        }
        printf("sweep_c_ok %d\nsweep_c_bad %lld\n", ok, k.bad);
    }
    return 0;
}
