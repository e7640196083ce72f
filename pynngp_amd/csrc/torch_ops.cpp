// PyTorch-ROCm operators over the C ABI of libnngp_hip.so: TORCH_LIBRARY(nngp, ...).
//
// The drop-in boundary the north_star names ("exposed to Python as a PyTorch-ROCm custom
// op so the SeqNNGP fit/sample surface is a drop-in") as a native op library: the
// schemas are registered with the dispatcher here, the CUDA (= HIP on ROCm; PyTorch's
// key name, not a compat layer) implementations call include/nngp.h directly on torch's
// current HIP stream, so a call from Python is one dispatcher hop into C++ -- no ctypes,
// no Python in between.  CPU tensors have no kernel registered: they raise (there is no
// CPU fallback).  pynngp_amd/ops.py loads this library and adds the fake (meta) kernels
// for tracing; pynngp_amd.sweep.ShardedLogLik and pynngp_amd.gibbs.SeqNNGP sweep through
// nngp::bf_sweep_out.
//
// Reference interfaces replaced (pyNNGP, /root/reference): knn_prior(_rows) <-
// NNGP._make_s_neighbor_sets nngp.py:49-62; knn_query <- _init_ws / _make_t_neighbor_sets
// nngp.py:45-47,64-71; bf_sweep(_out) <- _CNs/_Ccross/_Cs/_Bsi/_Fsi nngp.py:73-96 and the
// log-likelihood oneSample needs (nngp.py:98-101); bf_cross <- B_t / F_t at t not in S.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <limits>

#include "../../include/nngp.h"

namespace {

// Every op runs on the current stream of ITS TENSORS' device, under a device guard for that
// device (a tensor on cuda:1 while cuda:0 is current must not launch on cuda:0's stream).
void* stream(const at::Tensor& t) { return (void*)at::hip::getCurrentHIPStream(t.device().index()).stream(); }

void check_rc(int rc, const char* what) { TORCH_CHECK(rc == NNGP_OK, what, " failed (", rc, "): ", nngp_last_error()); }

void check_coords(const at::Tensor& c, const char* name) {
    TORCH_CHECK(c.is_cuda(), name, " must be a ROCm GPU tensor (there is no CPU fallback)");
    TORCH_CHECK(c.scalar_type() == at::kDouble && c.dim() == 2 && c.size(1) >= 1 && c.size(1) <= NNGP_MAX_DIM,
                name, " must be float64 (N, dim), 1 <= dim <= ", NNGP_MAX_DIM);
    TORCH_CHECK(c.is_contiguous(), name, " must be contiguous");
}

void check_same_device(const at::Tensor& a, const at::Tensor& b, const char* name) {
    TORCH_CHECK(b.device() == a.device(), name, " is on ", b.device(), ", expected ", a.device());
}

void check_f64(const c10::optional<at::Tensor>& t, at::IntArrayRef shape, const at::Tensor& like, const char* name) {
    if (!t.has_value()) return;
    TORCH_CHECK(t->scalar_type() == at::kDouble && t->sizes() == shape && t->is_contiguous(), name,
                " must be a contiguous float64 tensor of shape ", shape);
    check_same_device(like, *t, name);
}

void check_nbr(const at::Tensor& nbr, const at::Tensor& like) {
    TORCH_CHECK(nbr.scalar_type() == at::kInt && nbr.dim() == 2 && nbr.is_contiguous(),
                "nbr must be a contiguous int32 (rows, m) tensor");
    check_same_device(like, nbr, "nbr");
}

template <typename T>
T* ptr(const c10::optional<at::Tensor>& t) {
    return t.has_value() ? (T*)t->data_ptr() : nullptr;
}

// a sweep workspace's first 256 bytes (the pair kernel's header: tile count, fused-fold ticket) start at
// zero (include/nngp.h); the rest is scratch
at::Tensor workspace(int64_t bytes, const at::Tensor& like) {
    auto ws = at::empty({bytes > 256 ? bytes : 256}, like.options().dtype(at::kByte));
    ws.narrow(0, 0, 256).zero_();
    return ws;
}

// ---------------------------------------------------------------- neighbour sets
at::Tensor knn_prior(const at::Tensor& coords, int64_t m, int64_t q0, int64_t q1) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    const int64_t n = coords.size(0), d = coords.size(1);
    TORCH_CHECK(0 <= q0 && q0 <= q1 && q1 <= n, "query rows [", q0, ", ", q1, ") outside [0, ", n, ")");
    auto out = at::empty({q1 - q0, m}, coords.options().dtype(at::kInt));
    auto ws = workspace((int64_t)nngp_knn_workspace_bytes(n, (int32_t)d, (int32_t)m), coords);
    check_rc(nngp_knn_prior(coords.data_ptr<double>(), n, (int32_t)d, (int32_t)m, q0, q1, out.data_ptr<int32_t>(),
                            ws.data_ptr(), ws.numel(), stream(coords)),
             "nngp_knn_prior");
    return out;
}

at::Tensor knn_prior_rows(const at::Tensor& coords, int64_t m, const at::Tensor& rows) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    TORCH_CHECK(rows.scalar_type() == at::kInt && rows.dim() == 1 && rows.is_contiguous(), "rows must be int32 (n_rows,)");
    check_same_device(coords, rows, "rows");
    const int64_t n = coords.size(0), d = coords.size(1);
    auto out = at::empty({rows.size(0), m}, coords.options().dtype(at::kInt));
    auto ws = workspace((int64_t)nngp_knn_workspace_bytes(n, (int32_t)d, (int32_t)m), coords);
    check_rc(nngp_knn_prior_rows(coords.data_ptr<double>(), n, (int32_t)d, (int32_t)m, rows.data_ptr<int32_t>(),
                                 rows.size(0), out.data_ptr<int32_t>(), ws.data_ptr(), ws.numel(), stream(coords)),
             "nngp_knn_prior_rows");
    return out;
}

at::Tensor knn_query(const at::Tensor& ref, const at::Tensor& query, int64_t k) {
    check_coords(ref, "ref");
    const at::OptionalDeviceGuard guard(ref.device());
    check_coords(query, "query");
    check_same_device(ref, query, "query");
    TORCH_CHECK(ref.size(1) == query.size(1), "ref and query have different dimensions");
    const int64_t d = ref.size(1);
    auto out = at::empty({query.size(0), k}, ref.options().dtype(at::kInt));
    auto ws = workspace((int64_t)nngp_knn_workspace_bytes(ref.size(0), (int32_t)d, (int32_t)k), ref);
    check_rc(nngp_knn_query(ref.data_ptr<double>(), ref.size(0), (int32_t)d, query.data_ptr<double>(), query.size(0),
                            (int32_t)k, out.data_ptr<int32_t>(), ws.data_ptr(), ws.numel(), stream(ref)),
             "nngp_knn_query");
    return out;
}

// ---------------------------------------------------------------- the fused sweep
// out-variant: every output buffer is the caller's (the hot path: no allocation per sweep)
void bf_sweep_out(const at::Tensor& coords, const at::Tensor& nbr, const c10::optional<at::Tensor>& order, int64_t i0,
                  int64_t kind, double sigma2, double phi, double tau2, const c10::optional<at::Tensor>& values,
                  const c10::optional<at::Tensor>& B, const c10::optional<at::Tensor>& F,
                  const c10::optional<at::Tensor>& R, const at::Tensor& partials, const at::Tensor& ws,
                  int64_t algo, double nu, const c10::optional<at::Tensor>& plan,
                  const c10::optional<at::Tensor>& plan_info, const c10::optional<at::Tensor>& cert,
                  const c10::optional<at::Tensor>& cert_info) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0), d = coords.size(1);
    if (order.has_value()) {
        TORCH_CHECK(order->scalar_type() == at::kInt && order->sizes() == at::IntArrayRef{rows} && order->is_contiguous(),
                    "order must be a contiguous int32 (rows,) tensor");
        check_same_device(coords, *order, "order");
    }
    check_f64(values, {n}, coords, "values");
    check_f64(B, {rows, m}, coords, "B");
    check_f64(F, {rows}, coords, "F");
    check_f64(R, {rows}, coords, "R");
    check_f64(partials, {4}, coords, "partials");
    TORCH_CHECK(ws.is_contiguous(), "workspace must be contiguous");
    check_same_device(coords, ws, "workspace");
    if (plan.has_value()) {
        // a wave pair plan (pair_plan op): the pair kernel with every shared covariance evaluated once per wave
        TORCH_CHECK(plan_info.has_value() && plan_info->device().is_cpu() && plan_info->scalar_type() == at::kLong &&
                        plan_info->numel() == NNGP_PLAN_INFO_LEN && plan_info->is_contiguous(),
                    "plan_info must be the pair_plan op's CPU int64 (", NNGP_PLAN_INFO_LEN, ",) tensor");
        TORCH_CHECK(plan->scalar_type() == at::kByte && plan->is_contiguous(), "plan must be a contiguous uint8 tensor");
        check_same_device(coords, *plan, "plan");
        TORCH_CHECK(algo == NNGP_ALGO_AUTO || algo == NNGP_ALGO_PAIRB, "a pair plan runs the pair kernel (algo ", algo, ")");
        check_rc(nngp_bf_sweep_plan(coords.data_ptr<double>(), n, (int32_t)d, nbr.data_ptr<int32_t>(), ptr<int32_t>(order),
                                    rows, (int32_t)m, i0, (int32_t)kind, sigma2, phi, tau2, ptr<double>(values),
                                    ptr<double>(B), ptr<double>(F), ptr<double>(R), partials.data_ptr<double>(),
                                    ws.data_ptr(), (size_t)ws.nbytes(), plan->data_ptr(), (size_t)plan->nbytes(),
                                    plan_info->data_ptr<int64_t>(), stream(coords)),
                 "nngp_bf_sweep_plan");
        return;
    }
    if (cert.has_value()) {
        // a neighbour-set certificate (nbr_cert op): trusted tiles skip the index checks and clamps, same bits
        TORCH_CHECK(cert_info.has_value() && cert_info->device().is_cpu() && cert_info->scalar_type() == at::kLong &&
                        cert_info->numel() == NNGP_CERT_INFO_LEN && cert_info->is_contiguous(),
                    "cert_info must be the nbr_cert op's CPU int64 (", NNGP_CERT_INFO_LEN, ",) tensor");
        TORCH_CHECK(cert->scalar_type() == at::kByte && cert->is_contiguous(), "cert must be a contiguous uint8 tensor");
        check_same_device(coords, *cert, "cert");
        check_rc(nngp_bf_sweep_cert(coords.data_ptr<double>(), n, (int32_t)d, nbr.data_ptr<int32_t>(), ptr<int32_t>(order),
                                    rows, (int32_t)m, i0, (int32_t)kind, sigma2, phi, tau2, nu, ptr<double>(values),
                                    ptr<double>(B), ptr<double>(F), ptr<double>(R), partials.data_ptr<double>(),
                                    ws.data_ptr(), (size_t)ws.nbytes(), (int32_t)algo, cert->data_ptr(),
                                    (size_t)cert->nbytes(), cert_info->data_ptr<int64_t>(), stream(coords)),
                 "nngp_bf_sweep_cert");
        return;
    }
    check_rc(nngp_bf_sweep(coords.data_ptr<double>(), n, (int32_t)d, nbr.data_ptr<int32_t>(), ptr<int32_t>(order), rows,
                           (int32_t)m, i0, (int32_t)kind, sigma2, phi, tau2, nu, ptr<double>(values), ptr<double>(B),
                           ptr<double>(F), ptr<double>(R), partials.data_ptr<double>(), ws.data_ptr(),
                           (size_t)ws.nbytes(), (int32_t)algo, stream(coords)),
             "nngp_bf_sweep");
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_sweep(const at::Tensor& coords, const at::Tensor& nbr, int64_t i0,
                                                        int64_t kind, double sigma2, double phi, double tau2,
                                                        const c10::optional<at::Tensor>& values, bool want_bf,
                                                        int64_t algo, const c10::optional<at::Tensor>& order,
                                                        double nu) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1);
    auto f64 = coords.options();
    at::Tensor B = want_bf ? at::empty({rows, m}, f64) : at::empty({0, m}, f64);
    at::Tensor F = want_bf ? at::empty({rows}, f64) : at::empty({0}, f64);
    at::Tensor p = at::empty({4}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_workspace_bytes(rows, (int32_t)m, (int32_t)kind,
                                                               (int32_t)coords.size(1), (int32_t)algo), coords);
    bf_sweep_out(coords, nbr, order, i0, kind, sigma2, phi, tau2, values,
                 want_bf ? c10::optional<at::Tensor>(B) : c10::nullopt,
                 want_bf ? c10::optional<at::Tensor>(F) : c10::nullopt, c10::nullopt, p, ws, algo, nu, c10::nullopt,
                 c10::nullopt, c10::nullopt, c10::nullopt);
    return {B, F, p};
}

// analytic gradient sweep (nngp_bf_grad): (partials (4,), grad (3,), G (rows, 3) or (0, 3))
std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_grad(const at::Tensor& coords, const at::Tensor& nbr,
                                                       const c10::optional<at::Tensor>& order, int64_t i0, int64_t kind,
                                                       double sigma2, double phi, double tau2, const at::Tensor& values,
                                                       bool want_rows) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0);
    check_f64(values, {n}, coords, "values");
    if (order.has_value()) {
        TORCH_CHECK(order->scalar_type() == at::kInt && order->dim() == 1 && order->size(0) == rows &&
                        order->is_contiguous(), "order must be a contiguous int32 (rows,) tensor");
        check_same_device(coords, *order, "order");
    }
    auto f64 = coords.options();
    at::Tensor p = at::empty({4}, f64), g = at::empty({3}, f64);
    at::Tensor G = at::empty({want_rows ? rows : 0, 3}, f64);
    const int64_t need = (int64_t)nngp_bf_grad_workspace_bytes(rows, (int32_t)m);
    auto ws = at::empty({need > 256 ? need : 256}, f64.dtype(at::kByte));
    check_rc(nngp_bf_grad(coords.data_ptr<double>(), n, (int32_t)coords.size(1), nbr.data_ptr<int32_t>(),
                          ptr<int32_t>(order), rows, (int32_t)m, i0, (int32_t)kind, sigma2, phi, tau2,
                          values.data_ptr<double>(), want_rows ? G.data_ptr<double>() : nullptr, p.data_ptr<double>(),
                          g.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel(), stream(coords)),
             "nngp_bf_grad");
    return {p, g, G};
}

// per-axis gradient sweep (nngp_bf_grad_aniso): (partials (4,), grad (dim + 2,), G (rows, dim + 2) or (0, dim + 2))
std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_grad_aniso(const at::Tensor& coords, const at::Tensor& nbr,
                                                             const c10::optional<at::Tensor>& order, int64_t i0,
                                                             int64_t kind, double sigma2, at::ArrayRef<double> phi,
                                                             double tau2, const at::Tensor& values, bool want_rows) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0), d = coords.size(1);
    check_f64(values, {n}, coords, "values");
    TORCH_CHECK((int64_t)phi.size() == d, "phi has ", phi.size(), " entries for ", d, "-dimensional coordinates");
    if (order.has_value()) {
        TORCH_CHECK(order->scalar_type() == at::kInt && order->dim() == 1 && order->size(0) == rows &&
                        order->is_contiguous(), "order must be a contiguous int32 (rows,) tensor");
        check_same_device(coords, *order, "order");
    }
    auto f64 = coords.options();
    at::Tensor p = at::empty({4}, f64), g = at::empty({d + 2}, f64);
    at::Tensor G = at::empty({want_rows ? rows : 0, d + 2}, f64);
    const int64_t need = (int64_t)nngp_bf_grad_aniso_workspace_bytes(rows, (int32_t)m, (int32_t)d);
    auto ws = at::empty({need > 256 ? need : 256}, f64.dtype(at::kByte));
    check_rc(nngp_bf_grad_aniso(coords.data_ptr<double>(), n, (int32_t)d, nbr.data_ptr<int32_t>(), ptr<int32_t>(order),
                                rows, (int32_t)m, i0, (int32_t)kind, sigma2, phi.data(), tau2,
                                values.data_ptr<double>(), want_rows ? G.data_ptr<double>() : nullptr,
                                p.data_ptr<double>(), g.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel(),
                                stream(coords)),
             "nngp_bf_grad_aniso");
    return {p, g, G};
}

// general-nu Matern gradient sweep (nngp_bf_grad_matern): (partials (4,), grad (4,), G (rows, 4) or (0, 4))
std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_grad_matern(const at::Tensor& coords, const at::Tensor& nbr,
                                                              const c10::optional<at::Tensor>& order, int64_t i0,
                                                              double sigma2, double phi, double tau2, double nu,
                                                              const at::Tensor& values, bool want_rows) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0);
    check_f64(values, {n}, coords, "values");
    if (order.has_value()) {
        TORCH_CHECK(order->scalar_type() == at::kInt && order->dim() == 1 && order->size(0) == rows &&
                        order->is_contiguous(), "order must be a contiguous int32 (rows,) tensor");
        check_same_device(coords, *order, "order");
    }
    auto f64 = coords.options();
    at::Tensor p = at::empty({4}, f64), g = at::empty({4}, f64);
    at::Tensor G = at::empty({want_rows ? rows : 0, 4}, f64);
    const int64_t need = (int64_t)nngp_bf_grad_matern_workspace_bytes(rows, (int32_t)m);
    auto ws = at::empty({need > 256 ? need : 256}, f64.dtype(at::kByte));
    check_rc(nngp_bf_grad_matern(coords.data_ptr<double>(), n, (int32_t)coords.size(1), nbr.data_ptr<int32_t>(),
                                 ptr<int32_t>(order), rows, (int32_t)m, i0, sigma2, phi, tau2, nu,
                                 values.data_ptr<double>(), want_rows ? G.data_ptr<double>() : nullptr,
                                 p.data_ptr<double>(), g.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel(),
                                 stream(coords)),
             "nngp_bf_grad_matern");
    return {p, g, G};
}

// u rho'(u) and d rho / d nu of the Matern correlation through the sweep's derivative table (nngp_matern_eval_d)
std::tuple<at::Tensor, at::Tensor> matern_eval_d(const at::Tensor& u, double nu) {
    TORCH_CHECK(u.scalar_type() == at::kDouble && u.is_contiguous(), "u must be a contiguous float64 tensor");
    const at::OptionalDeviceGuard guard(u.device());
    at::Tensor h = at::empty_like(u), dnu = at::empty_like(u);
    check_rc(nngp_matern_eval_d(u.data_ptr<double>(), u.numel(), nu, h.data_ptr<double>(), dnu.data_ptr<double>(),
                                stream(u)),
             "nngp_matern_eval_d");
    return {h, dnu};
}

// the factors and their phi-derivatives (nngp_bf_dphi): (B (rows, m), F (rows,), dB (rows, m), dF (rows,), partials (4,))
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> bf_dphi(
    const at::Tensor& coords, const at::Tensor& nbr, const c10::optional<at::Tensor>& order, int64_t i0, int64_t kind,
    double sigma2, double phi, double tau2) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0);
    if (order.has_value()) {
        TORCH_CHECK(order->scalar_type() == at::kInt && order->dim() == 1 && order->size(0) == rows &&
                        order->is_contiguous(), "order must be a contiguous int32 (rows,) tensor");
        check_same_device(coords, *order, "order");
    }
    auto f64 = coords.options();
    at::Tensor B = at::empty({rows, m}, f64), F = at::empty({rows}, f64);
    at::Tensor dB = at::empty({rows, m}, f64), dF = at::empty({rows}, f64), p = at::empty({4}, f64);
    const int64_t need = (int64_t)nngp_bf_dphi_workspace_bytes(rows, (int32_t)m);
    auto ws = at::empty({need > 256 ? need : 256}, f64.dtype(at::kByte));
    check_rc(nngp_bf_dphi(coords.data_ptr<double>(), n, (int32_t)coords.size(1), nbr.data_ptr<int32_t>(),
                          ptr<int32_t>(order), rows, (int32_t)m, i0, (int32_t)kind, sigma2, phi, tau2,
                          B.data_ptr<double>(), F.data_ptr<double>(), dB.data_ptr<double>(), dF.data_ptr<double>(),
                          p.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel(), stream(coords)),
             "nngp_bf_dphi");
    return {B, F, dB, dF, p};
}

// Fisher information sweep (nngp_bf_fisher): (partials (4,), grad (3,), info (6,), I_rows (rows, 6) or (0, 6),
// G (rows, 3) or (0, 3)); values None: the information alone
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> bf_fisher(
    const at::Tensor& coords, const at::Tensor& nbr, const c10::optional<at::Tensor>& order, int64_t i0, int64_t kind,
    double sigma2, double phi, double tau2, const c10::optional<at::Tensor>& values, bool want_rows) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0);
    if (values.has_value()) check_f64(*values, {n}, coords, "values");
    if (order.has_value()) {
        TORCH_CHECK(order->scalar_type() == at::kInt && order->dim() == 1 && order->size(0) == rows &&
                        order->is_contiguous(), "order must be a contiguous int32 (rows,) tensor");
        check_same_device(coords, *order, "order");
    }
    auto f64 = coords.options();
    at::Tensor p = at::empty({4}, f64), g = at::empty({3}, f64), info = at::empty({6}, f64);
    at::Tensor I = at::empty({want_rows ? rows : 0, 6}, f64), G = at::empty({want_rows ? rows : 0, 3}, f64);
    const int64_t need = (int64_t)nngp_bf_fisher_workspace_bytes(rows, (int32_t)m);
    auto ws = at::empty({need > 256 ? need : 256}, f64.dtype(at::kByte));
    check_rc(nngp_bf_fisher(coords.data_ptr<double>(), n, (int32_t)coords.size(1), nbr.data_ptr<int32_t>(),
                            ptr<int32_t>(order), rows, (int32_t)m, i0, (int32_t)kind, sigma2, phi, tau2,
                            ptr<double>(values), want_rows ? I.data_ptr<double>() : nullptr,
                            want_rows ? G.data_ptr<double>() : nullptr, p.data_ptr<double>(), g.data_ptr<double>(),
                            info.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel(), stream(coords)),
             "nngp_bf_fisher");
    return {p, g, info, I, G};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_cross(const at::Tensor& ref, const at::Tensor& query,
                                                        const at::Tensor& nbr, int64_t kind, double sigma2, double phi,
                                                        double tau2, const c10::optional<at::Tensor>& ref_values,
                                                        int64_t algo, double nu) {
    check_coords(ref, "ref");
    const at::OptionalDeviceGuard guard(ref.device());
    check_coords(query, "query");
    check_same_device(ref, query, "query");
    TORCH_CHECK(ref.size(1) == query.size(1), "ref and query have different dimensions");
    check_nbr(nbr, ref);
    const int64_t rows = nbr.size(0), m = nbr.size(1), d = ref.size(1);
    check_f64(ref_values, {ref.size(0)}, ref, "ref_values");
    auto f64 = ref.options();
    at::Tensor B = at::empty({rows, m}, f64), F = at::empty({rows}, f64), R = at::empty({rows}, f64);
    at::Tensor p = at::empty({4}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_workspace_bytes(rows, (int32_t)m, (int32_t)kind, (int32_t)d,
                                                               (int32_t)algo), ref);
    check_rc(nngp_bf_cross(ref.data_ptr<double>(), ref.size(0), (int32_t)d, query.data_ptr<double>(), query.size(0),
                           nbr.data_ptr<int32_t>(), nullptr, rows, (int32_t)m, 0, (int32_t)kind, sigma2, phi, tau2,
                           nu, ptr<double>(ref_values), nullptr, B.data_ptr<double>(), F.data_ptr<double>(),
                           ref_values.has_value() ? R.data_ptr<double>() : nullptr, p.data_ptr<double>(),
                           ws.data_ptr(), ws.nbytes(), (int32_t)algo, stream(ref)),
             "nngp_bf_cross");
    // R = 0 - B_t v_N: the kriging mean is -R (zeros without reference values)
    at::Tensor mean = ref_values.has_value() ? R.neg() : at::zeros({rows}, f64);
    return {B, F, mean};
}

// ---------------------------------------------------------------- per-point noise (nngp_bf_*_noise)
static void check_order(const c10::optional<at::Tensor>& order, int64_t rows, const at::Tensor& like) {
    if (!order.has_value()) return;
    TORCH_CHECK(order->scalar_type() == at::kInt && order->dim() == 1 && order->size(0) == rows && order->is_contiguous(),
                "order must be a contiguous int32 (rows,) tensor");
    check_same_device(like, *order, "order");
}

// (B (rows, m), F (rows,), R (rows,), partials (4,)); B, F empty without want_bf, R empty without values
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> bf_sweep_noise(
    const at::Tensor& coords, const at::Tensor& nbr, const c10::optional<at::Tensor>& order, int64_t i0, int64_t kind,
    double sigma2, double phi, double tau2, const c10::optional<at::Tensor>& values, const at::Tensor& noise_var,
    bool want_bf) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0);
    check_f64(values, {n}, coords, "values");
    check_f64(noise_var, {n}, coords, "noise_var");
    check_order(order, rows, coords);
    auto f64 = coords.options();
    const bool wr = values.has_value();
    at::Tensor B = at::empty({want_bf ? rows : 0, m}, f64), F = at::empty({want_bf ? rows : 0}, f64);
    at::Tensor R = at::empty({wr ? rows : 0}, f64), p = at::empty({4}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_noise_workspace_bytes(rows, (int32_t)m), coords);
    check_rc(nngp_bf_sweep_noise(coords.data_ptr<double>(), n, (int32_t)coords.size(1), nbr.data_ptr<int32_t>(),
                                 ptr<int32_t>(order), rows, (int32_t)m, i0, (int32_t)kind, sigma2, phi, tau2,
                                 ptr<double>(values), noise_var.data_ptr<double>(), want_bf ? B.data_ptr<double>() : nullptr,
                                 want_bf ? F.data_ptr<double>() : nullptr, wr ? R.data_ptr<double>() : nullptr,
                                 p.data_ptr<double>(), ws.data_ptr(), (size_t)ws.nbytes(), stream(coords)),
             "nngp_bf_sweep_noise");
    return {B, F, R, p};
}

// (partials (4,), grad (3,), G (rows, 3) or (0, 3)), as bf_grad
std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_grad_noise(const at::Tensor& coords, const at::Tensor& nbr,
                                                             const c10::optional<at::Tensor>& order, int64_t i0,
                                                             int64_t kind, double sigma2, double phi, double tau2,
                                                             const at::Tensor& values, const at::Tensor& noise_var,
                                                             bool want_rows) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0);
    check_f64(values, {n}, coords, "values");
    check_f64(noise_var, {n}, coords, "noise_var");
    check_order(order, rows, coords);
    auto f64 = coords.options();
    at::Tensor p = at::empty({4}, f64), g = at::empty({3}, f64);
    at::Tensor G = at::empty({want_rows ? rows : 0, 3}, f64);
    const int64_t need = (int64_t)nngp_bf_grad_workspace_bytes(rows, (int32_t)m);
    auto ws = at::empty({need > 256 ? need : 256}, f64.dtype(at::kByte));
    check_rc(nngp_bf_grad_noise(coords.data_ptr<double>(), n, (int32_t)coords.size(1), nbr.data_ptr<int32_t>(),
                                ptr<int32_t>(order), rows, (int32_t)m, i0, (int32_t)kind, sigma2, phi, tau2,
                                values.data_ptr<double>(), noise_var.data_ptr<double>(),
                                want_rows ? G.data_ptr<double>() : nullptr, p.data_ptr<double>(), g.data_ptr<double>(),
                                ws.data_ptr(), (size_t)ws.numel(), stream(coords)),
             "nngp_bf_grad_noise");
    return {p, g, G};
}

// (B, F, kriging mean), as bf_cross
std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_cross_noise(const at::Tensor& ref, const at::Tensor& query,
                                                              const at::Tensor& nbr, int64_t kind, double sigma2,
                                                              double phi, double tau2,
                                                              const c10::optional<at::Tensor>& ref_values,
                                                              const at::Tensor& noise_ref,
                                                              const c10::optional<at::Tensor>& noise_query) {
    check_coords(ref, "ref");
    const at::OptionalDeviceGuard guard(ref.device());
    check_coords(query, "query");
    check_same_device(ref, query, "query");
    TORCH_CHECK(ref.size(1) == query.size(1), "ref and query have different dimensions");
    check_nbr(nbr, ref);
    const int64_t rows = nbr.size(0), m = nbr.size(1), d = ref.size(1);
    check_f64(ref_values, {ref.size(0)}, ref, "ref_values");
    check_f64(noise_ref, {ref.size(0)}, ref, "noise_ref");
    check_f64(noise_query, {query.size(0)}, ref, "noise_query");
    auto f64 = ref.options();
    at::Tensor B = at::empty({rows, m}, f64), F = at::empty({rows}, f64), R = at::empty({rows}, f64);
    at::Tensor p = at::empty({4}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_noise_workspace_bytes(rows, (int32_t)m), ref);
    check_rc(nngp_bf_cross_noise(ref.data_ptr<double>(), ref.size(0), (int32_t)d, query.data_ptr<double>(), query.size(0),
                                 nbr.data_ptr<int32_t>(), nullptr, rows, (int32_t)m, 0, (int32_t)kind, sigma2, phi, tau2,
                                 ptr<double>(ref_values), nullptr, noise_ref.data_ptr<double>(), ptr<double>(noise_query),
                                 B.data_ptr<double>(), F.data_ptr<double>(),
                                 ref_values.has_value() ? R.data_ptr<double>() : nullptr, p.data_ptr<double>(),
                                 ws.data_ptr(), ws.nbytes(), stream(ref)),
             "nngp_bf_cross_noise");
    at::Tensor mean = ref_values.has_value() ? R.neg() : at::zeros({rows}, f64);
    return {B, F, mean};
}

// ---------------------------------------------------------------- separable space-time (nngp_bf_*_sep)
// (B (rows, m), F (rows,), R (rows,), partials (4,)); B, F empty without want_bf, R empty without values
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> bf_sweep_sep(
    const at::Tensor& coords, const at::Tensor& nbr, const c10::optional<at::Tensor>& order, int64_t i0, int64_t kind_s,
    int64_t kind_t, double sigma2, double phi_s, double phi_t, double tau2, const c10::optional<at::Tensor>& values,
    bool want_bf) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0);
    check_f64(values, {n}, coords, "values");
    check_order(order, rows, coords);
    auto f64 = coords.options();
    const bool wr = values.has_value();
    at::Tensor B = at::empty({want_bf ? rows : 0, m}, f64), F = at::empty({want_bf ? rows : 0}, f64);
    at::Tensor R = at::empty({wr ? rows : 0}, f64), p = at::empty({4}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_sep_workspace_bytes(rows, (int32_t)m), coords);
    check_rc(nngp_bf_sweep_sep(coords.data_ptr<double>(), n, (int32_t)coords.size(1), nbr.data_ptr<int32_t>(),
                               ptr<int32_t>(order), rows, (int32_t)m, i0, (int32_t)kind_s, (int32_t)kind_t, sigma2, phi_s,
                               phi_t, tau2, ptr<double>(values), want_bf ? B.data_ptr<double>() : nullptr,
                               want_bf ? F.data_ptr<double>() : nullptr, wr ? R.data_ptr<double>() : nullptr,
                               p.data_ptr<double>(), ws.data_ptr(), (size_t)ws.nbytes(), stream(coords)),
             "nngp_bf_sweep_sep");
    return {B, F, R, p};
}

// (partials (4,), grad (4,) in (sigma2, phi_s, phi_t, tau2), G (rows, 4) or (0, 4))
std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_grad_sep(const at::Tensor& coords, const at::Tensor& nbr,
                                                           const c10::optional<at::Tensor>& order, int64_t i0,
                                                           int64_t kind_s, int64_t kind_t, double sigma2, double phi_s,
                                                           double phi_t, double tau2, const at::Tensor& values,
                                                           bool want_rows) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0);
    check_f64(values, {n}, coords, "values");
    check_order(order, rows, coords);
    auto f64 = coords.options();
    at::Tensor p = at::empty({4}, f64), g = at::empty({4}, f64);
    at::Tensor G = at::empty({want_rows ? rows : 0, 4}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_sep_workspace_bytes(rows, (int32_t)m), coords);
    check_rc(nngp_bf_grad_sep(coords.data_ptr<double>(), n, (int32_t)coords.size(1), nbr.data_ptr<int32_t>(),
                              ptr<int32_t>(order), rows, (int32_t)m, i0, (int32_t)kind_s, (int32_t)kind_t, sigma2, phi_s,
                              phi_t, tau2, values.data_ptr<double>(), want_rows ? G.data_ptr<double>() : nullptr,
                              p.data_ptr<double>(), g.data_ptr<double>(), ws.data_ptr(), (size_t)ws.nbytes(),
                              stream(coords)),
             "nngp_bf_grad_sep");
    return {p, g, G};
}

// (B, F, kriging mean), as bf_cross
std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_cross_sep(const at::Tensor& ref, const at::Tensor& query,
                                                            const at::Tensor& nbr, int64_t kind_s, int64_t kind_t,
                                                            double sigma2, double phi_s, double phi_t, double tau2,
                                                            const c10::optional<at::Tensor>& ref_values) {
    check_coords(ref, "ref");
    const at::OptionalDeviceGuard guard(ref.device());
    check_coords(query, "query");
    check_same_device(ref, query, "query");
    TORCH_CHECK(ref.size(1) == query.size(1), "ref and query have different dimensions");
    check_nbr(nbr, ref);
    const int64_t rows = nbr.size(0), m = nbr.size(1), d = ref.size(1);
    check_f64(ref_values, {ref.size(0)}, ref, "ref_values");
    auto f64 = ref.options();
    at::Tensor B = at::empty({rows, m}, f64), F = at::empty({rows}, f64), R = at::empty({rows}, f64);
    at::Tensor p = at::empty({4}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_sep_workspace_bytes(rows, (int32_t)m), ref);
    check_rc(nngp_bf_cross_sep(ref.data_ptr<double>(), ref.size(0), (int32_t)d, query.data_ptr<double>(), query.size(0),
                               nbr.data_ptr<int32_t>(), nullptr, rows, (int32_t)m, 0, (int32_t)kind_s, (int32_t)kind_t,
                               sigma2, phi_s, phi_t, tau2, ptr<double>(ref_values), nullptr, B.data_ptr<double>(),
                               F.data_ptr<double>(), ref_values.has_value() ? R.data_ptr<double>() : nullptr,
                               p.data_ptr<double>(), ws.data_ptr(), ws.nbytes(), stream(ref)),
             "nngp_bf_cross_sep");
    at::Tensor mean = ref_values.has_value() ? R.neg() : at::zeros({rows}, f64);
    return {B, F, mean};
}

// ---------------------------------------------------------------- points in 4 .. 16 dimensions (nngp_*_nd)
void check_coords_nd(const at::Tensor& c, const char* name) {
    TORCH_CHECK(c.is_cuda(), name, " must be a ROCm GPU tensor (there is no CPU fallback)");
    TORCH_CHECK(c.scalar_type() == at::kDouble && c.dim() == 2 && c.size(1) > NNGP_MAX_DIM && c.size(1) <= NNGP_ND_MAX_DIM,
                name, " must be float64 (N, dim), ", NNGP_MAX_DIM + 1, " <= dim <= ", NNGP_ND_MAX_DIM);
    TORCH_CHECK(c.is_contiguous(), name, " must be contiguous");
}

void check_phi_nd(at::ArrayRef<double> phi, const at::Tensor& coords) {
    TORCH_CHECK((int64_t)phi.size() == coords.size(1), "phi must hold one decay per coordinate column (", coords.size(1),
                "), got ", phi.size());
}

at::Tensor knn_prior_nd(const at::Tensor& coords, int64_t m, int64_t q0, int64_t q1) {
    check_coords_nd(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    const int64_t n = coords.size(0), d = coords.size(1);
    TORCH_CHECK(0 <= q0 && q0 <= q1 && q1 <= n, "query rows [", q0, ", ", q1, ") outside [0, ", n, ")");
    auto out = at::empty({q1 - q0, m}, coords.options().dtype(at::kInt));
    auto ws = workspace((int64_t)nngp_knn_nd_workspace_bytes(n, (int32_t)d, (int32_t)m), coords);
    check_rc(nngp_knn_prior_nd(coords.data_ptr<double>(), n, (int32_t)d, (int32_t)m, q0, q1, out.data_ptr<int32_t>(),
                               ws.data_ptr(), ws.numel(), stream(coords)),
             "nngp_knn_prior_nd");
    return out;
}

at::Tensor knn_query_nd(const at::Tensor& ref, const at::Tensor& query, int64_t k) {
    check_coords_nd(ref, "ref");
    const at::OptionalDeviceGuard guard(ref.device());
    check_coords_nd(query, "query");
    check_same_device(ref, query, "query");
    TORCH_CHECK(ref.size(1) == query.size(1), "ref and query have different dimensions");
    const int64_t d = ref.size(1);
    auto out = at::empty({query.size(0), k}, ref.options().dtype(at::kInt));
    auto ws = workspace((int64_t)nngp_knn_nd_workspace_bytes(ref.size(0), (int32_t)d, (int32_t)k), ref);
    check_rc(nngp_knn_query_nd(ref.data_ptr<double>(), ref.size(0), (int32_t)d, query.data_ptr<double>(), query.size(0),
                               (int32_t)k, out.data_ptr<int32_t>(), ws.data_ptr(), ws.numel(), stream(ref)),
             "nngp_knn_query_nd");
    return out;
}

// (B (rows, m), F (rows,), R (rows,), partials (4,)); B, F empty without want_bf, R empty without values
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> bf_sweep_nd(
    const at::Tensor& coords, const at::Tensor& nbr, const c10::optional<at::Tensor>& order, int64_t i0, int64_t kind,
    double sigma2, at::ArrayRef<double> phi, double tau2, const c10::optional<at::Tensor>& values, bool want_bf) {
    check_coords_nd(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    check_phi_nd(phi, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0), d = coords.size(1);
    check_f64(values, {n}, coords, "values");
    check_order(order, rows, coords);
    auto f64 = coords.options();
    const bool wr = values.has_value();
    at::Tensor B = at::empty({want_bf ? rows : 0, m}, f64), F = at::empty({want_bf ? rows : 0}, f64);
    at::Tensor R = at::empty({wr ? rows : 0}, f64), p = at::empty({4}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_nd_workspace_bytes(rows, (int32_t)m, (int32_t)d), coords);
    check_rc(nngp_bf_sweep_nd(coords.data_ptr<double>(), n, (int32_t)d, nbr.data_ptr<int32_t>(), ptr<int32_t>(order), rows,
                              (int32_t)m, i0, (int32_t)kind, sigma2, phi.data(), tau2, ptr<double>(values),
                              want_bf ? B.data_ptr<double>() : nullptr, want_bf ? F.data_ptr<double>() : nullptr,
                              wr ? R.data_ptr<double>() : nullptr, p.data_ptr<double>(), ws.data_ptr(),
                              (size_t)ws.nbytes(), stream(coords)),
             "nngp_bf_sweep_nd");
    return {B, F, R, p};
}

// (partials (4,), grad (dim + 2,) in (sigma2, phi_1..phi_dim, tau2), G (rows, dim + 2) or (0, dim + 2))
std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_grad_nd(const at::Tensor& coords, const at::Tensor& nbr,
                                                          const c10::optional<at::Tensor>& order, int64_t i0,
                                                          int64_t kind, double sigma2, at::ArrayRef<double> phi,
                                                          double tau2, const at::Tensor& values, bool want_rows) {
    check_coords_nd(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    check_phi_nd(phi, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0), d = coords.size(1);
    check_f64(values, {n}, coords, "values");
    check_order(order, rows, coords);
    auto f64 = coords.options();
    at::Tensor p = at::empty({4}, f64), g = at::empty({d + 2}, f64);
    at::Tensor G = at::empty({want_rows ? rows : 0, d + 2}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_nd_workspace_bytes(rows, (int32_t)m, (int32_t)d), coords);
    check_rc(nngp_bf_grad_nd(coords.data_ptr<double>(), n, (int32_t)d, nbr.data_ptr<int32_t>(), ptr<int32_t>(order), rows,
                             (int32_t)m, i0, (int32_t)kind, sigma2, phi.data(), tau2, values.data_ptr<double>(),
                             want_rows ? G.data_ptr<double>() : nullptr, p.data_ptr<double>(), g.data_ptr<double>(),
                             ws.data_ptr(), (size_t)ws.nbytes(), stream(coords)),
             "nngp_bf_grad_nd");
    return {p, g, G};
}

// (B, F, kriging mean), as bf_cross
std::tuple<at::Tensor, at::Tensor, at::Tensor> bf_cross_nd(const at::Tensor& ref, const at::Tensor& query,
                                                           const at::Tensor& nbr, int64_t kind, double sigma2,
                                                           at::ArrayRef<double> phi, double tau2,
                                                           const c10::optional<at::Tensor>& ref_values) {
    check_coords_nd(ref, "ref");
    const at::OptionalDeviceGuard guard(ref.device());
    check_coords_nd(query, "query");
    check_same_device(ref, query, "query");
    TORCH_CHECK(ref.size(1) == query.size(1), "ref and query have different dimensions");
    check_nbr(nbr, ref);
    check_phi_nd(phi, ref);
    const int64_t rows = nbr.size(0), m = nbr.size(1), d = ref.size(1);
    check_f64(ref_values, {ref.size(0)}, ref, "ref_values");
    auto f64 = ref.options();
    at::Tensor B = at::empty({rows, m}, f64), F = at::empty({rows}, f64), R = at::empty({rows}, f64);
    at::Tensor p = at::empty({4}, f64);
    auto ws = workspace((int64_t)nngp_bf_sweep_nd_workspace_bytes(rows, (int32_t)m, (int32_t)d), ref);
    check_rc(nngp_bf_cross_nd(ref.data_ptr<double>(), ref.size(0), (int32_t)d, query.data_ptr<double>(), query.size(0),
                              nbr.data_ptr<int32_t>(), nullptr, rows, (int32_t)m, 0, (int32_t)kind, sigma2, phi.data(),
                              tau2, ptr<double>(ref_values), nullptr, B.data_ptr<double>(), F.data_ptr<double>(),
                              ref_values.has_value() ? R.data_ptr<double>() : nullptr, p.data_ptr<double>(),
                              ws.data_ptr(), ws.nbytes(), stream(ref)),
             "nngp_bf_cross_nd");
    at::Tensor mean = ref_values.has_value() ? R.neg() : at::zeros({rows}, f64);
    return {B, F, mean};
}

// the wave pair plan of a sweep over nbr (include/nngp.h nngp_pair_plan_build): (plan bytes on the GPU,
// CPU int64 info).  A setup call: it synchronises the tensors' stream once.
std::tuple<at::Tensor, at::Tensor> pair_plan(const at::Tensor& nbr, const c10::optional<at::Tensor>& order, int64_t i0,
                                             int64_t n_points, int64_t dim) {
    TORCH_CHECK(nbr.is_cuda(), "nbr must be a ROCm GPU tensor (there is no CPU fallback)");
    const at::OptionalDeviceGuard guard(nbr.device());
    check_nbr(nbr, nbr);
    const int64_t rows = nbr.size(0), m = nbr.size(1);
    if (order.has_value()) {
        TORCH_CHECK(order->scalar_type() == at::kInt && order->sizes() == at::IntArrayRef{rows} && order->is_contiguous(),
                    "order must be a contiguous int32 (rows,) tensor");
        check_same_device(nbr, *order, "order");
    }
    const size_t bytes = nngp_pair_plan_bytes(rows, (int32_t)m, (int32_t)dim);
    TORCH_CHECK(bytes > 0, "no pair plans for m=", m, ", dim=", dim, " (2 <= m <= 17, dim 1..3)");
    auto plan = workspace((int64_t)bytes, nbr);
    auto info = at::empty({NNGP_PLAN_INFO_LEN}, at::TensorOptions().dtype(at::kLong));
    check_rc(nngp_pair_plan_build(nbr.data_ptr<int32_t>(), ptr<int32_t>(order), rows, (int32_t)m, i0, n_points,
                                  (int32_t)dim, plan.data_ptr(), (size_t)plan.nbytes(), info.data_ptr<int64_t>(),
                                  stream(nbr)),
             "nngp_pair_plan_build");
    return {plan, info};
}

// the neighbour-set certificate of a sweep over (coords, nbr, order, i0) (include/nngp.h nngp_nbr_cert_build):
// (certificate bytes on the GPU, CPU int64 info).  A setup call: it synchronises the tensors' stream once.
std::tuple<at::Tensor, at::Tensor> nbr_cert(const at::Tensor& coords, const at::Tensor& nbr,
                                            const c10::optional<at::Tensor>& order, int64_t i0) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    check_nbr(nbr, coords);
    const int64_t rows = nbr.size(0), m = nbr.size(1), n = coords.size(0), d = coords.size(1);
    if (order.has_value()) {
        TORCH_CHECK(order->scalar_type() == at::kInt && order->sizes() == at::IntArrayRef{rows} && order->is_contiguous(),
                    "order must be a contiguous int32 (rows,) tensor");
        check_same_device(coords, *order, "order");
    }
    auto cert = workspace((int64_t)nngp_nbr_cert_bytes(rows), coords);
    auto info = at::empty({NNGP_CERT_INFO_LEN}, at::TensorOptions().dtype(at::kLong));
    check_rc(nngp_nbr_cert_build(coords.data_ptr<double>(), n, (int32_t)d, nbr.data_ptr<int32_t>(), ptr<int32_t>(order),
                                 rows, (int32_t)m, i0, cert.data_ptr(), (size_t)cert.nbytes(), info.data_ptr<int64_t>(),
                                 stream(coords)),
             "nngp_nbr_cert_build");
    return {cert, info};
}

std::tuple<at::Tensor, at::Tensor> row_order(const at::Tensor& coords, int64_t i0, int64_t rows,
                                             const c10::optional<at::Tensor>& nbr) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    const int64_t n = coords.size(0);
    TORCH_CHECK(0 <= i0 && 0 <= rows && i0 + rows <= n, "rows [", i0, ", ", i0 + rows, ") outside [0, ", n, ")");
    int64_t m = 0;
    if (nbr.has_value()) {
        check_nbr(*nbr, coords);
        TORCH_CHECK(nbr->size(0) == rows, "nbr must have one row per location");
        m = nbr->size(1);
    }
    auto order = at::empty({rows}, coords.options().dtype(at::kInt));
    at::Tensor srt = nbr.has_value() ? at::empty_like(*nbr) : at::empty({0, 0}, coords.options().dtype(at::kInt));
    auto ws = workspace((int64_t)nngp_row_order_workspace_bytes(rows), coords);
    check_rc(nngp_row_order(coords.data_ptr<double>(), n, (int32_t)coords.size(1), ptr<int32_t>(nbr), (int32_t)m, i0,
                            rows, order.data_ptr<int32_t>(), nbr.has_value() ? srt.data_ptr<int32_t>() : nullptr,
                            ws.data_ptr(), ws.nbytes(), stream(coords)),
             "nngp_row_order");
    return {order, srt};
}

// levelled max-min order (nngp_order_maxmin): (perm int64 (n,), level int32 (n,)); a setup call (it synchronises
// the stream once per round)
std::tuple<at::Tensor, at::Tensor> order_maxmin(const at::Tensor& coords, int64_t seed) {
    check_coords(coords, "coords");
    const at::OptionalDeviceGuard guard(coords.device());
    const int64_t n = coords.size(0);
    TORCH_CHECK(n >= 1, "order_maxmin needs at least one point");
    TORCH_CHECK(seed >= 0 && seed <= (int64_t)std::numeric_limits<uint32_t>::max(), "seed must be a uint32");
    auto perm = at::empty({n}, coords.options().dtype(at::kLong));
    auto level = at::empty({n}, coords.options().dtype(at::kInt));
    auto ws = workspace((int64_t)nngp_order_maxmin_workspace_bytes(n, (int32_t)coords.size(1)), coords);
    check_rc(nngp_order_maxmin(coords.data_ptr<double>(), n, (int32_t)coords.size(1), (uint32_t)seed,
                               perm.data_ptr<int64_t>(), level.data_ptr<int32_t>(), ws.data_ptr(), ws.nbytes(),
                               stream(coords)),
             "nngp_order_maxmin");
    return {perm, level};
}

// gathered (world, 4) -> out (4,), or a batch of independent sweeps: gathered (world, n_slots, 4) -> out (n_slots, 4)
void combine_partials_out(const at::Tensor& gathered, const at::Tensor& out) {
    TORCH_CHECK(gathered.is_cuda() && gathered.scalar_type() == at::kDouble &&
                    (gathered.dim() == 2 || gathered.dim() == 3) && gathered.size(-1) == 4 && gathered.is_contiguous(),
                "gathered must be a contiguous float64 (world, 4) or (world, n_slots, 4) GPU tensor");
    const at::OptionalDeviceGuard guard(gathered.device());
    const int64_t slots = gathered.dim() == 3 ? gathered.size(1) : 1;
    if (gathered.dim() == 3)
        check_f64(out, {slots, 4}, gathered, "out");
    else
        check_f64(out, {4}, gathered, "out");
    check_rc(nngp_combine_partials_batch(gathered.data_ptr<double>(), (int32_t)gathered.size(0), slots,
                                         out.data_ptr<double>(), stream(gathered)),
             "nngp_combine_partials_batch");
}

// ---------------------------------------------------------------- latent-field posterior
// the shared argument checks of precision_apply / latent_cg (raw pointers below: every length is checked)
void check_latent(const at::Tensor& nbr, const at::Tensor& B, const at::Tensor& off, const at::Tensor& rev_j,
                  const at::Tensor& rev_k, const at::Tensor& prep) {
    TORCH_CHECK(nbr.is_cuda(), "nbr must be a ROCm GPU tensor (there is no CPU fallback)");
    check_nbr(nbr, nbr);
    const int64_t n = nbr.size(0), m = nbr.size(1);
    TORCH_CHECK(m >= 1 && m <= NNGP_MAX_M, "m=", m, " outside [1, ", NNGP_MAX_M, "]");
    check_f64(B, {n, m}, nbr, "B");
    TORCH_CHECK(off.scalar_type() == at::kInt && off.dim() == 1 && off.size(0) == n + 1 && off.is_contiguous(),
                "off must be a contiguous int32 (n + 1,) tensor");
    check_same_device(nbr, off, "off");
    for (const at::Tensor* t : {&rev_j, &rev_k}) {
        TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) >= n * m && t->is_contiguous(),
                    "rev_j / rev_k must be contiguous int32 tensors of at least n * m entries");
        check_same_device(nbr, *t, "rev_j / rev_k");
    }
    TORCH_CHECK(prep.scalar_type() == at::kByte && prep.is_contiguous() &&
                    (size_t)prep.numel() >= nngp_gibbs_prep_bytes(n, (int32_t)m),
                "prep must be the contiguous uint8 buffer of nngp_gibbs_prepare for these factors");
    check_same_device(nbr, prep, "prep");
}

// out = [(I - B)^T (sigma2 F)^-1 (I - B) + diag(d)] x (nngp_precision_apply)
at::Tensor precision_apply(const at::Tensor& nbr, const at::Tensor& B, const at::Tensor& off, const at::Tensor& rev_j,
                           const at::Tensor& rev_k, const at::Tensor& prep, double sigma2,
                           const c10::optional<at::Tensor>& d, const at::Tensor& x) {
    check_latent(nbr, B, off, rev_j, rev_k, prep);
    const at::OptionalDeviceGuard guard(nbr.device());
    const int64_t n = nbr.size(0), m = nbr.size(1);
    check_f64(d, {n}, nbr, "d");
    check_f64(x, {n}, nbr, "x");
    auto out = at::empty_like(x);
    auto ws = at::empty({(int64_t)nngp_precision_workspace_bytes(n)}, nbr.options().dtype(at::kByte));
    check_rc(nngp_precision_apply(nbr.data_ptr<int32_t>(), B.data_ptr<double>(), off.data_ptr<int32_t>(),
                                  rev_j.data_ptr<int32_t>(), rev_k.data_ptr<int32_t>(), prep.data_ptr(), n, (int32_t)m,
                                  sigma2, ptr<double>(d), x.data_ptr<double>(), out.data_ptr<double>(), ws.data_ptr(),
                                  (size_t)ws.nbytes(), stream(nbr)),
             "nngp_precision_apply");
    return out;
}

// Jacobi-PCG for A x = b (nngp_latent_cg; synchronises once per check_every iterations): (x, info), info a
// CPU float64 (4,): iterations, converged (1 / 0 / -1 breakdown), |r|^2, |b|^2
std::tuple<at::Tensor, at::Tensor> latent_cg(const at::Tensor& nbr, const at::Tensor& B, const at::Tensor& off,
                                             const at::Tensor& rev_j, const at::Tensor& rev_k, const at::Tensor& prep,
                                             double sigma2, const c10::optional<at::Tensor>& d, const at::Tensor& b,
                                             const c10::optional<at::Tensor>& x0, double rtol, int64_t max_iter,
                                             int64_t check_every) {
    check_latent(nbr, B, off, rev_j, rev_k, prep);
    const at::OptionalDeviceGuard guard(nbr.device());
    const int64_t n = nbr.size(0), m = nbr.size(1);
    check_f64(d, {n}, nbr, "d");
    check_f64(b, {n}, nbr, "b");
    check_f64(x0, {n}, nbr, "x0");
    at::Tensor x = x0.has_value() ? x0->clone() : at::zeros_like(b);
    auto info = at::empty({4}, at::TensorOptions().dtype(at::kDouble));
    auto ws = at::empty({(int64_t)nngp_latent_cg_workspace_bytes(n)}, nbr.options().dtype(at::kByte));
    check_rc(nngp_latent_cg(nbr.data_ptr<int32_t>(), B.data_ptr<double>(), off.data_ptr<int32_t>(),
                            rev_j.data_ptr<int32_t>(), rev_k.data_ptr<int32_t>(), prep.data_ptr(), n, (int32_t)m, sigma2,
                            ptr<double>(d), b.data_ptr<double>(), x.data_ptr<double>(), rtol, max_iter,
                            (int32_t)check_every, info.data_ptr<double>(), ws.data_ptr(), (size_t)ws.nbytes(),
                            stream(nbr)),
             "nngp_latent_cg");
    return {x, info};
}

// the batched forms: x / b / x0 (n, nrhs), 1 <= nrhs <= NNGP_LATENT_MAX_RHS; column c bit-identical to the single op
int64_t check_batch(const at::Tensor& v, const at::Tensor& nbr, const char* name) {
    TORCH_CHECK(v.dim() == 2 && v.size(1) >= 1 && v.size(1) <= NNGP_LATENT_MAX_RHS, name,
                " must be (n, nrhs) with 1 <= nrhs <= ", NNGP_LATENT_MAX_RHS);
    check_f64(v, {nbr.size(0), v.size(1)}, nbr, name);
    return v.size(1);
}

at::Tensor precision_apply_batch(const at::Tensor& nbr, const at::Tensor& B, const at::Tensor& off,
                                 const at::Tensor& rev_j, const at::Tensor& rev_k, const at::Tensor& prep,
                                 double sigma2, const c10::optional<at::Tensor>& d, const at::Tensor& x) {
    check_latent(nbr, B, off, rev_j, rev_k, prep);
    const at::OptionalDeviceGuard guard(nbr.device());
    const int64_t n = nbr.size(0), m = nbr.size(1);
    check_f64(d, {n}, nbr, "d");
    const int64_t nrhs = check_batch(x, nbr, "x");
    auto out = at::empty_like(x);
    auto ws = at::empty({(int64_t)nngp_precision_batch_workspace_bytes(n, (int32_t)nrhs)},
                        nbr.options().dtype(at::kByte));
    check_rc(nngp_precision_apply_batch(nbr.data_ptr<int32_t>(), B.data_ptr<double>(), off.data_ptr<int32_t>(),
                                        rev_j.data_ptr<int32_t>(), rev_k.data_ptr<int32_t>(), prep.data_ptr(), n,
                                        (int32_t)m, sigma2, ptr<double>(d), (int32_t)nrhs, x.data_ptr<double>(),
                                        out.data_ptr<double>(), ws.data_ptr(), (size_t)ws.nbytes(), stream(nbr)),
             "nngp_precision_apply_batch");
    return out;
}

// (x (n, nrhs), info): info a CPU float64 (nrhs, 4), row c as latent_cg's info of column c
std::tuple<at::Tensor, at::Tensor> latent_cg_batch(const at::Tensor& nbr, const at::Tensor& B, const at::Tensor& off,
                                                   const at::Tensor& rev_j, const at::Tensor& rev_k,
                                                   const at::Tensor& prep, double sigma2,
                                                   const c10::optional<at::Tensor>& d, const at::Tensor& b,
                                                   const c10::optional<at::Tensor>& x0, double rtol, int64_t max_iter,
                                                   int64_t check_every) {
    check_latent(nbr, B, off, rev_j, rev_k, prep);
    const at::OptionalDeviceGuard guard(nbr.device());
    const int64_t n = nbr.size(0), m = nbr.size(1);
    check_f64(d, {n}, nbr, "d");
    const int64_t nrhs = check_batch(b, nbr, "b");
    check_f64(x0, {n, nrhs}, nbr, "x0");
    at::Tensor x = x0.has_value() ? x0->clone() : at::zeros_like(b);
    auto info = at::empty({nrhs, 4}, at::TensorOptions().dtype(at::kDouble));
    auto ws = at::empty({(int64_t)nngp_latent_cg_batch_workspace_bytes(n, (int32_t)nrhs)},
                        nbr.options().dtype(at::kByte));
    check_rc(nngp_latent_cg_batch(nbr.data_ptr<int32_t>(), B.data_ptr<double>(), off.data_ptr<int32_t>(),
                                  rev_j.data_ptr<int32_t>(), rev_k.data_ptr<int32_t>(), prep.data_ptr(), n, (int32_t)m,
                                  sigma2, ptr<double>(d), (int32_t)nrhs, b.data_ptr<double>(), x.data_ptr<double>(),
                                  rtol, max_iter, (int32_t)check_every, info.data_ptr<double>(), ws.data_ptr(),
                                  (size_t)ws.nbytes(), stream(nbr)),
             "nngp_latent_cg_batch");
    return {x, info};
}

// latent_cg_batch with the solver's scalars recorded (nngp_latent_ref_cg_batch_trace at n_s = n): (x, info, trace),
// trace a device float64 (nrhs, max_iter, 2) filled with NaN, trace[c][k] = (alpha_k, beta_k) for every iteration
// k column c completed -- the Lanczos tridiagonal of M^-1/2 A M^-1/2.  x and info are latent_cg_batch's, bit for bit
std::tuple<at::Tensor, at::Tensor, at::Tensor> latent_cg_batch_trace(
    const at::Tensor& nbr, const at::Tensor& B, const at::Tensor& off, const at::Tensor& rev_j,
    const at::Tensor& rev_k, const at::Tensor& prep, double sigma2, const c10::optional<at::Tensor>& d,
    const at::Tensor& b, const c10::optional<at::Tensor>& x0, double rtol, int64_t max_iter, int64_t check_every) {
    check_latent(nbr, B, off, rev_j, rev_k, prep);
    const at::OptionalDeviceGuard guard(nbr.device());
    const int64_t n = nbr.size(0), m = nbr.size(1);
    check_f64(d, {n}, nbr, "d");
    const int64_t nrhs = check_batch(b, nbr, "b");
    check_f64(x0, {n, nrhs}, nbr, "x0");
    TORCH_CHECK(max_iter >= 0, "max_iter must be >= 0");
    at::Tensor x = x0.has_value() ? x0->clone() : at::zeros_like(b);
    auto info = at::empty({nrhs, 4}, at::TensorOptions().dtype(at::kDouble));
    auto trace = at::full({nrhs, max_iter, 2}, std::numeric_limits<double>::quiet_NaN(), b.options());
    auto ws = at::empty({(int64_t)nngp_latent_ref_cg_batch_workspace_bytes(n, n, (int32_t)nrhs)},
                        nbr.options().dtype(at::kByte));
    check_rc(nngp_latent_ref_cg_batch_trace(nbr.data_ptr<int32_t>(), B.data_ptr<double>(), off.data_ptr<int32_t>(),
                                            rev_j.data_ptr<int32_t>(), rev_k.data_ptr<int32_t>(), prep.data_ptr(), n,
                                            n, (int32_t)m, sigma2, ptr<double>(d), (int32_t)nrhs,
                                            b.data_ptr<double>(), x.data_ptr<double>(), rtol, max_iter,
                                            (int32_t)check_every, info.data_ptr<double>(), ws.data_ptr(),
                                            (size_t)ws.nbytes(), trace.data_ptr<double>(), max_iter, stream(nbr)),
             "nngp_latent_ref_cg_batch_trace");
    return {x, info, trace};
}

// ---------------------------------------------------------------- Polya-Gamma draws (binomial model)
// omega ~ PG(trials, c) per location and the status word (0 = clean, else the smallest index + 1 whose draw is
// NaN: a non-finite c, trials outside [0, NNGP_PG_MAX_TRIALS] or a loop cap -- faults are data, the op does not
// synchronise to read it)
std::tuple<at::Tensor, at::Tensor> polya_gamma(const at::Tensor& trials, const at::Tensor& c, int64_t seed,
                                               int64_t sweep) {
    TORCH_CHECK(trials.is_cuda() && c.is_cuda(), "trials and c must be ROCm GPU tensors (there is no CPU fallback)");
    const at::OptionalDeviceGuard guard(c.device());
    check_same_device(c, trials, "trials");
    TORCH_CHECK(trials.scalar_type() == at::kInt && trials.dim() == 1 && trials.is_contiguous(),
                "trials must be a contiguous int32 (n,) tensor");
    TORCH_CHECK(c.scalar_type() == at::kDouble && c.dim() == 1 && c.is_contiguous() && c.size(0) == trials.size(0),
                "c must be a contiguous float64 (n,) tensor");
    TORCH_CHECK(sweep >= 0 && sweep < ((int64_t)1 << 40), "sweep must lie in [0, 2^40)");
    auto omega = at::empty_like(c);
    auto status = at::empty({1}, c.options().dtype(at::kInt));
    check_rc(nngp_polya_gamma(c.size(0), trials.data_ptr<int32_t>(), c.data_ptr<double>(), (uint64_t)seed,
                              (uint64_t)sweep, omega.data_ptr<double>(), status.data_ptr<int32_t>(), stream(c)),
             "nngp_polya_gamma");
    return {omega, status};
}

// ---------------------------------------------------------------- binomial latent posterior (Laplace)
// One Newton step's link quantities per node: (d, rhs, g, partials); partials = (sum l, max |g|, first node with a
// non-finite offset + w, + 1, or 0; first node with negative trials, + 1, or 0) -- faults are data, no synchronisation
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> binomial_newton_step(const at::Tensor& trials,
                                                                                const at::Tensor& successes,
                                                                                const at::Tensor& offset,
                                                                                const at::Tensor& w) {
    TORCH_CHECK(trials.is_cuda() && successes.is_cuda() && offset.is_cuda() && w.is_cuda(),
                "trials, successes, offset and w must be ROCm GPU tensors (there is no CPU fallback)");
    const at::OptionalDeviceGuard guard(w.device());
    check_same_device(w, trials, "trials");
    TORCH_CHECK(trials.scalar_type() == at::kInt && trials.dim() == 1 && trials.is_contiguous(),
                "trials must be a contiguous int32 (n,) tensor");
    const int64_t n = trials.size(0);
    check_f64(successes, {n}, w, "successes");
    check_f64(offset, {n}, w, "offset");
    check_f64(w, {n}, w, "w");
    auto d = at::empty_like(w), rhs = at::empty_like(w), g = at::empty_like(w);
    auto partials = at::empty({4}, w.options());
    auto ws = workspace((int64_t)nngp_binomial_newton_step_workspace_bytes(n), w);
    check_rc(nngp_binomial_newton_step(n, trials.data_ptr<int32_t>(), successes.data_ptr<double>(),
                                       offset.data_ptr<double>(), w.data_ptr<double>(), d.data_ptr<double>(),
                                       rhs.data_ptr<double>(), g.data_ptr<double>(), partials.data_ptr<double>(),
                                       ws.data_ptr(), (size_t)ws.nbytes(), stream(w)),
             "nngp_binomial_newton_step");
    return {d, rhs, g, partials};
}

// E[logistic(mu + s Z)], Z ~ N(0, 1), per element
at::Tensor logistic_normal(const at::Tensor& mu, const at::Tensor& s) {
    TORCH_CHECK(mu.is_cuda() && s.is_cuda(), "mu and s must be ROCm GPU tensors (there is no CPU fallback)");
    const at::OptionalDeviceGuard guard(mu.device());
    TORCH_CHECK(mu.scalar_type() == at::kDouble && mu.dim() == 1 && mu.is_contiguous(),
                "mu must be a contiguous float64 (n,) tensor");
    check_f64(s, {mu.size(0)}, mu, "s");
    auto out = at::empty_like(mu);
    check_rc(nngp_logistic_normal(mu.size(0), mu.data_ptr<double>(), s.data_ptr<double>(), out.data_ptr<double>(),
                                  stream(mu)),
             "nngp_logistic_normal");
    return out;
}

// ---------------------------------------------------------------- solves with the NNGP factor
// one level schedule of nngp_factor_levels: rows / level_off on the device, level_off_host a CPU copy
struct FactorSched {
    const int32_t *rows, *level_off, *level_off_host;
    int64_t n_levels;
};
FactorSched check_sched(const at::Tensor& nbr, const at::Tensor& rows, const at::Tensor& level_off,
                        const at::Tensor& level_off_host) {
    const int64_t n = nbr.size(0);
    TORCH_CHECK(rows.scalar_type() == at::kInt && rows.dim() == 1 && rows.size(0) == n && rows.is_contiguous(),
                "rows must be a contiguous int32 (n,) tensor");
    check_same_device(nbr, rows, "rows");
    TORCH_CHECK(level_off_host.device().is_cpu() && level_off_host.scalar_type() == at::kInt &&
                    level_off_host.dim() == 1 && level_off_host.size(0) >= 1 && level_off_host.is_contiguous(),
                "level_off_host must be a contiguous CPU int32 (n_levels + 1,) tensor");
    TORCH_CHECK(level_off.scalar_type() == at::kInt && level_off.dim() == 1 &&
                    level_off.size(0) == level_off_host.size(0) && level_off.is_contiguous(),
                "level_off must be a contiguous int32 tensor of level_off_host's length");
    check_same_device(nbr, level_off, "level_off");
    return {rows.data_ptr<int32_t>(), level_off.data_ptr<int32_t>(), level_off_host.data_ptr<int32_t>(),
            level_off_host.size(0) - 1};
}

// x = (I - B)^-1 b, or (I - B)^-T b for trans (nngp_factor_solve_batch); b (n, nrhs)
at::Tensor factor_solve(const at::Tensor& nbr, const at::Tensor& B, const at::Tensor& off, const at::Tensor& rev_j,
                        const at::Tensor& rev_k, const at::Tensor& prep, const at::Tensor& rows,
                        const at::Tensor& level_off, const at::Tensor& level_off_host, bool trans, int64_t fuse_width,
                        const at::Tensor& b) {
    check_latent(nbr, B, off, rev_j, rev_k, prep);
    const at::OptionalDeviceGuard guard(nbr.device());
    const int64_t n = nbr.size(0), m = nbr.size(1);
    const FactorSched sc = check_sched(nbr, rows, level_off, level_off_host);
    const int64_t nrhs = check_batch(b, nbr, "b");
    TORCH_CHECK(fuse_width >= 0 && fuse_width <= NNGP_FACTOR_MAX_FUSE_WIDTH, "fuse_width outside [0, ",
                NNGP_FACTOR_MAX_FUSE_WIDTH, "]");
    auto x = at::empty_like(b);
    check_rc(nngp_factor_solve_batch(nbr.data_ptr<int32_t>(), B.data_ptr<double>(), off.data_ptr<int32_t>(),
                                     rev_j.data_ptr<int32_t>(), rev_k.data_ptr<int32_t>(), prep.data_ptr(), sc.rows,
                                     sc.level_off, sc.level_off_host, sc.n_levels, n, (int32_t)m, (int32_t)nrhs,
                                     trans ? 1 : 0, (int32_t)fuse_width, b.data_ptr<double>(), x.data_ptr<double>(),
                                     stream(nbr)),
             "nngp_factor_solve_batch");
    return x;
}

// out = sigma2 (I - B)^-1 F (I - B)^-T v (nngp_factor_cov_apply_batch); v (n, nrhs)
at::Tensor factor_cov_apply(const at::Tensor& nbr, const at::Tensor& B, const at::Tensor& F, const at::Tensor& off,
                            const at::Tensor& rev_j, const at::Tensor& rev_k, const at::Tensor& prep,
                            const at::Tensor& rows_f, const at::Tensor& level_off_f, const at::Tensor& level_off_f_host,
                            const at::Tensor& rows_t, const at::Tensor& level_off_t, const at::Tensor& level_off_t_host,
                            double sigma2, int64_t fuse_width, const at::Tensor& v) {
    check_latent(nbr, B, off, rev_j, rev_k, prep);
    const at::OptionalDeviceGuard guard(nbr.device());
    const int64_t n = nbr.size(0), m = nbr.size(1);
    check_f64(F, {n}, nbr, "F");
    const FactorSched sf = check_sched(nbr, rows_f, level_off_f, level_off_f_host);
    const FactorSched st = check_sched(nbr, rows_t, level_off_t, level_off_t_host);
    const int64_t nrhs = check_batch(v, nbr, "v");
    TORCH_CHECK(fuse_width >= 0 && fuse_width <= NNGP_FACTOR_MAX_FUSE_WIDTH, "fuse_width outside [0, ",
                NNGP_FACTOR_MAX_FUSE_WIDTH, "]");
    auto out = at::empty_like(v);
    check_rc(nngp_factor_cov_apply_batch(nbr.data_ptr<int32_t>(), B.data_ptr<double>(), F.data_ptr<double>(),
                                         off.data_ptr<int32_t>(), rev_j.data_ptr<int32_t>(), rev_k.data_ptr<int32_t>(),
                                         prep.data_ptr(), sf.rows, sf.level_off, sf.level_off_host, sf.n_levels,
                                         st.rows, st.level_off, st.level_off_host, st.n_levels, n, (int32_t)m, sigma2,
                                         (int32_t)nrhs, (int32_t)fuse_width, v.data_ptr<double>(),
                                         out.data_ptr<double>(), stream(nbr)),
             "nngp_factor_cov_apply_batch");
    return out;
}

// ---------------------------------------------------------------- whitened Gram sweep
// U = F^-1/2 (I - B) V and, with want_gram, G = U^T U (nngp_whiten_gram); V (n_points, ncol <= 16); Vq: the values
// at the rows themselves for query rows against a reference set (None: S = T, the rows are points i0 ..)
std::tuple<at::Tensor, at::Tensor> whiten_gram(const at::Tensor& nbr, const c10::optional<at::Tensor>& order,
                                               const at::Tensor& B, const at::Tensor& F, int64_t i0,
                                               const at::Tensor& V, const c10::optional<at::Tensor>& Vq,
                                               bool want_gram) {
    TORCH_CHECK(nbr.is_cuda() && B.is_cuda() && F.is_cuda() && V.is_cuda(),
                "nbr, B, F and V must be ROCm GPU tensors (there is no CPU fallback)");
    const at::OptionalDeviceGuard guard(nbr.device());
    check_nbr(nbr, V);
    const int64_t n = nbr.size(0), m = nbr.size(1);
    check_f64(B, {n, m}, nbr, "B");
    check_f64(F, {n}, nbr, "F");
    TORCH_CHECK(V.scalar_type() == at::kDouble && V.dim() == 2 && V.is_contiguous() && V.size(1) >= 1 &&
                    V.size(1) <= NNGP_WHITEN_MAX_COLS,
                "V must be a contiguous float64 (n_points, ncol) tensor, 1 <= ncol <= ", NNGP_WHITEN_MAX_COLS);
    const int64_t ncol = V.size(1);
    check_f64(Vq, {n, ncol}, nbr, "Vq");
    if (order.has_value()) {
        TORCH_CHECK(order->scalar_type() == at::kInt && order->dim() == 1 && order->size(0) == n &&
                        order->is_contiguous(), "order must be a contiguous int32 (rows,) tensor");
        check_same_device(nbr, *order, "order");
    }
    auto U = at::empty({n, ncol}, V.options());
    auto gram = at::empty({want_gram ? ncol : 0, want_gram ? ncol : 0}, V.options());
    auto ws = workspace((int64_t)nngp_whiten_gram_workspace_bytes(n, (int32_t)ncol), V);
    check_rc(nngp_whiten_gram(nbr.data_ptr<int32_t>(), ptr<int32_t>(order), B.data_ptr<double>(), F.data_ptr<double>(),
                              n, (int32_t)m, i0, V.size(0), (int32_t)ncol, V.data_ptr<double>(), ptr<double>(Vq),
                              U.data_ptr<double>(), want_gram ? gram.data_ptr<double>() : nullptr, ws.data_ptr(),
                              ws.numel(), stream(nbr)),
             "nngp_whiten_gram");
    return {U, gram};
}

}  // namespace

TORCH_LIBRARY(nngp, m) {
    m.def("whiten_gram(Tensor nbr, Tensor? order, Tensor B, Tensor F, int i0, Tensor V, Tensor? Vq, bool want_gram) "
          "-> (Tensor, Tensor)");
    m.def("factor_solve(Tensor nbr, Tensor B, Tensor off, Tensor rev_j, Tensor rev_k, Tensor prep, Tensor rows, "
          "Tensor level_off, Tensor level_off_host, bool trans, int fuse_width, Tensor b) -> Tensor");
    m.def("factor_cov_apply(Tensor nbr, Tensor B, Tensor F, Tensor off, Tensor rev_j, Tensor rev_k, Tensor prep, "
          "Tensor rows_f, Tensor level_off_f, Tensor level_off_f_host, Tensor rows_t, Tensor level_off_t, "
          "Tensor level_off_t_host, float sigma2, int fuse_width, Tensor v) -> Tensor");
    m.def("binomial_newton_step(Tensor trials, Tensor successes, Tensor offset, Tensor w) -> "
          "(Tensor, Tensor, Tensor, Tensor)");
    m.def("logistic_normal(Tensor mu, Tensor s) -> Tensor");
    m.def("precision_apply_batch(Tensor nbr, Tensor B, Tensor off, Tensor rev_j, Tensor rev_k, Tensor prep, "
          "float sigma2, Tensor? d, Tensor x) -> Tensor");
    m.def("latent_cg_batch(Tensor nbr, Tensor B, Tensor off, Tensor rev_j, Tensor rev_k, Tensor prep, float sigma2, "
          "Tensor? d, Tensor b, Tensor? x0=None, float rtol=1e-08, int max_iter=1000, int check_every=8) -> "
          "(Tensor, Tensor)");
    m.def("latent_cg_batch_trace(Tensor nbr, Tensor B, Tensor off, Tensor rev_j, Tensor rev_k, Tensor prep, "
          "float sigma2, Tensor? d, Tensor b, Tensor? x0=None, float rtol=1e-08, int max_iter=1000, "
          "int check_every=8) -> (Tensor, Tensor, Tensor)");
    m.def("precision_apply(Tensor nbr, Tensor B, Tensor off, Tensor rev_j, Tensor rev_k, Tensor prep, float sigma2, "
          "Tensor? d, Tensor x) -> Tensor");
    m.def("latent_cg(Tensor nbr, Tensor B, Tensor off, Tensor rev_j, Tensor rev_k, Tensor prep, float sigma2, "
          "Tensor? d, Tensor b, Tensor? x0=None, float rtol=1e-08, int max_iter=1000, int check_every=8) -> "
          "(Tensor, Tensor)");
    m.def("polya_gamma(Tensor trials, Tensor c, int seed, int sweep) -> (Tensor, Tensor)");
    m.def("knn_prior(Tensor coords, int m, int q0, int q1) -> Tensor");
    m.def("knn_prior_rows(Tensor coords, int m, Tensor rows) -> Tensor");
    m.def("knn_query(Tensor ref, Tensor query, int k) -> Tensor");
    m.def("bf_sweep(Tensor coords, Tensor nbr, int i0, int kind, float sigma2, float phi, float tau2, Tensor? values, "
          "bool want_bf, int algo, Tensor? order=None, float nu=-1.0) -> (Tensor, Tensor, Tensor)");
    m.def("bf_sweep_out(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind, float sigma2, float phi, "
          "float tau2, Tensor? values, Tensor(a!)? B, Tensor(b!)? F, Tensor(c!)? R, Tensor(d!) partials, "
          "Tensor(e!) workspace, int algo, float nu=-1.0, Tensor? plan=None, Tensor? plan_info=None, "
          "Tensor? cert=None, Tensor? cert_info=None) -> ()");
    m.def("bf_grad(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind, float sigma2, float phi, float tau2, "
          "Tensor values, bool want_rows) -> (Tensor, Tensor, Tensor)");
    m.def("bf_grad_aniso(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind, float sigma2, float[] phi, "
          "float tau2, Tensor values, bool want_rows) -> (Tensor, Tensor, Tensor)");
    m.def("bf_grad_matern(Tensor coords, Tensor nbr, Tensor? order, int i0, float sigma2, float phi, float tau2, "
          "float nu, Tensor values, bool want_rows) -> (Tensor, Tensor, Tensor)");
    m.def("matern_eval_d(Tensor u, float nu) -> (Tensor, Tensor)");
    m.def("bf_dphi(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind, float sigma2, float phi, float tau2) "
          "-> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("bf_fisher(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind, float sigma2, float phi, float tau2, "
          "Tensor? values, bool want_rows) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("nbr_cert(Tensor coords, Tensor nbr, Tensor? order, int i0) -> (Tensor, Tensor)");
    m.def("pair_plan(Tensor nbr, Tensor? order, int i0, int n_points, int dim) -> (Tensor, Tensor)");
    m.def("bf_cross(Tensor ref, Tensor query, Tensor nbr, int kind, float sigma2, float phi, float tau2, "
          "Tensor? ref_values, int algo, float nu=-1.0) -> (Tensor, Tensor, Tensor)");
    m.def("bf_sweep_noise(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind, float sigma2, float phi, "
          "float tau2, Tensor? values, Tensor noise_var, bool want_bf) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("bf_grad_noise(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind, float sigma2, float phi, "
          "float tau2, Tensor values, Tensor noise_var, bool want_rows) -> (Tensor, Tensor, Tensor)");
    m.def("bf_cross_noise(Tensor ref, Tensor query, Tensor nbr, int kind, float sigma2, float phi, float tau2, "
          "Tensor? ref_values, Tensor noise_ref, Tensor? noise_query) -> (Tensor, Tensor, Tensor)");
    m.def("bf_sweep_sep(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind_s, int kind_t, float sigma2, "
          "float phi_s, float phi_t, float tau2, Tensor? values, bool want_bf) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("bf_grad_sep(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind_s, int kind_t, float sigma2, "
          "float phi_s, float phi_t, float tau2, Tensor values, bool want_rows) -> (Tensor, Tensor, Tensor)");
    m.def("bf_cross_sep(Tensor ref, Tensor query, Tensor nbr, int kind_s, int kind_t, float sigma2, float phi_s, "
          "float phi_t, float tau2, Tensor? ref_values) -> (Tensor, Tensor, Tensor)");
    m.def("knn_prior_nd(Tensor coords, int m, int q0, int q1) -> Tensor");
    m.def("knn_query_nd(Tensor ref, Tensor query, int k) -> Tensor");
    m.def("bf_sweep_nd(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind, float sigma2, float[] phi, "
          "float tau2, Tensor? values, bool want_bf) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("bf_grad_nd(Tensor coords, Tensor nbr, Tensor? order, int i0, int kind, float sigma2, float[] phi, "
          "float tau2, Tensor values, bool want_rows) -> (Tensor, Tensor, Tensor)");
    m.def("bf_cross_nd(Tensor ref, Tensor query, Tensor nbr, int kind, float sigma2, float[] phi, float tau2, "
          "Tensor? ref_values) -> (Tensor, Tensor, Tensor)");
    m.def("row_order(Tensor coords, int i0, int rows, Tensor? nbr) -> (Tensor, Tensor)");
    m.def("order_maxmin(Tensor coords, int seed) -> (Tensor, Tensor)");
    m.def("combine_partials_out(Tensor gathered, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(nngp, CUDA, m) {
    m.impl("polya_gamma", &polya_gamma);
    m.impl("binomial_newton_step", &binomial_newton_step);
    m.impl("logistic_normal", &logistic_normal);
    m.impl("knn_prior", &knn_prior);
    m.impl("knn_prior_rows", &knn_prior_rows);
    m.impl("knn_query", &knn_query);
    m.impl("bf_sweep", &bf_sweep);
    m.impl("bf_sweep_out", &bf_sweep_out);
    m.impl("bf_cross", &bf_cross);
    m.impl("bf_grad", &bf_grad);
    m.impl("bf_sweep_noise", &bf_sweep_noise);
    m.impl("bf_grad_noise", &bf_grad_noise);
    m.impl("bf_cross_noise", &bf_cross_noise);
    m.impl("bf_sweep_sep", &bf_sweep_sep);
    m.impl("bf_grad_sep", &bf_grad_sep);
    m.impl("bf_cross_sep", &bf_cross_sep);
    m.impl("knn_prior_nd", &knn_prior_nd);
    m.impl("knn_query_nd", &knn_query_nd);
    m.impl("bf_sweep_nd", &bf_sweep_nd);
    m.impl("bf_grad_nd", &bf_grad_nd);
    m.impl("bf_cross_nd", &bf_cross_nd);
    m.impl("bf_grad_aniso", &bf_grad_aniso);
    m.impl("bf_grad_matern", &bf_grad_matern);
    m.impl("matern_eval_d", &matern_eval_d);
    m.impl("bf_dphi", &bf_dphi);
    m.impl("bf_fisher", &bf_fisher);
    m.impl("row_order", &row_order);
    m.impl("order_maxmin", &order_maxmin);
    m.impl("pair_plan", &pair_plan);
    m.impl("nbr_cert", &nbr_cert);
    m.impl("combine_partials_out", &combine_partials_out);
    m.impl("precision_apply", &precision_apply);
    m.impl("latent_cg", &latent_cg);
    m.impl("precision_apply_batch", &precision_apply_batch);
    m.impl("factor_solve", &factor_solve);
    m.impl("factor_cov_apply", &factor_cov_apply);
    m.impl("latent_cg_batch", &latent_cg_batch);
    m.impl("latent_cg_batch_trace", &latent_cg_batch_trace);
    m.impl("whiten_gram", &whiten_gram);
}
