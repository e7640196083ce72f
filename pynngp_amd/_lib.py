"""ctypes binding of ``libnngp_hip.so`` (the C ABI in ``include/nngp.h``).

This is the only place that touches the native library.  It loads the in-tree
build (``pynngp_amd/_build/libnngp_hip.so``, made by ``__graft_entry__.build()``
or ``make -C pynngp_amd/csrc``) and fails loudly when it is missing or when a
tensor is not on a ROCm GPU: there is no CPU fallback for the hot path.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# NNGP_LIB overrides the library path (A/B timing of alternative builds only; it must exist)
LIB_PATH = os.environ.get("NNGP_LIB") or os.path.join(_HERE, "_build", "libnngp_hip.so")
SYMBOLS = (
    "nngp_version",
    "nngp_abi_version",
    "nngp_last_error",
    "nngp_knn_workspace_bytes",
    "nngp_knn_prior",
    "nngp_knn_prior_rows",
    "nngp_knn_query",
    "nngp_bf_sweep_workspace_bytes",
    "nngp_bf_sweep",
    "nngp_bf_cross",
    "nngp_bf_finalize",
    "nngp_resolve_algo",
    "nngp_resolve_algo_nu",
    "nngp_loglik_from_partials",
    "nngp_check_partials",
    "nngp_row_order_workspace_bytes",
    "nngp_row_order",
    "nngp_combine_partials",
    "nngp_combine_partials_batch",
    "nngp_matern_eval",
    "nngp_joint_entries",
    "nngp_joint_dist",
    "nngp_bf_sweep_blocks_workspace_bytes",
    "nngp_bf_sweep_blocks",
    "nngp_reverse_workspace_bytes",
    "nngp_reverse_neighbors",
    "nngp_color_moral_graph",
    "nngp_gibbs_prep_bytes",
    "nngp_gibbs_prepare",
    "nngp_gibbs_member_rows",
    "nngp_gibbs_w_sweep",
    "nngp_gibbs_normals",
    "nngp_gibbs_prepare_range",
    "nngp_gibbs_w_color",
    "nngp_gibbs_w_color_dev",
    "nngp_gibbs_w_apply",
    "nngp_gibbs_stats_workspace_bytes",
    "nngp_gibbs_stats",
    "nngp_gibbs_w_sweep_chains",
    "nngp_gibbs_w_sweep_chains_il",
    "nngp_gibbs_w_sweep_tiles",
    "nngp_color_moral_graph_dev",
    "nngp_pair_plan_supported",
    "nngp_pair_plan_bytes",
    "nngp_pair_plan_build",
    "nngp_bf_sweep_plan",
    "nngp_nbr_cert_bytes",
    "nngp_nbr_cert_build",
    "nngp_nbr_cert_trusted_tiles",
    "nngp_bf_sweep_cert",
    "nngp_bf_grad_workspace_bytes",
    "nngp_bf_grad",
    "nngp_bf_sweep_noise_workspace_bytes",
    "nngp_bf_sweep_noise",
    "nngp_bf_cross_noise",
    "nngp_bf_grad_noise",
    "nngp_bf_sweep_sep_workspace_bytes",
    "nngp_bf_sweep_sep",
    "nngp_bf_cross_sep",
    "nngp_bf_grad_sep",
    "nngp_knn_nd_workspace_bytes",
    "nngp_knn_prior_nd",
    "nngp_knn_query_nd",
    "nngp_bf_sweep_nd_workspace_bytes",
    "nngp_bf_sweep_nd",
    "nngp_bf_cross_nd",
    "nngp_bf_grad_nd",
    "nngp_bf_grad_aniso_workspace_bytes",
    "nngp_bf_grad_aniso",
    "nngp_bf_grad_matern_workspace_bytes",
    "nngp_bf_grad_matern",
    "nngp_matern_eval_d",
    "nngp_bf_dphi_workspace_bytes",
    "nngp_bf_dphi",
    "nngp_bf_fisher_workspace_bytes",
    "nngp_bf_fisher",
    "nngp_precision_workspace_bytes",
    "nngp_precision_apply",
    "nngp_precision_sqrt_t_apply",
    "nngp_latent_cg_workspace_bytes",
    "nngp_latent_cg",
    "nngp_precision_batch_workspace_bytes",
    "nngp_precision_apply_batch",
    "nngp_precision_sqrt_t_apply_batch",
    "nngp_latent_cg_batch_workspace_bytes",
    "nngp_latent_cg_batch",
    "nngp_precision_diag",
    "nngp_precision_ref_batch_workspace_bytes",
    "nngp_precision_ref_apply_batch",
    "nngp_precision_ref_sqrt_t_apply_batch",
    "nngp_precision_ref_fold_batch",
    "nngp_precision_ref_diag",
    "nngp_latent_ref_cg_batch_workspace_bytes",
    "nngp_latent_ref_cg_batch",
    "nngp_latent_ref_cg_batch_trace",
    "nngp_latent_ref_leaves_batch",
    "nngp_latent_rows_dot2_batch",
    "nngp_polya_gamma",
    "nngp_gibbs_pg_update",
    "nngp_gibbs_pg_stats_workspace_bytes",
    "nngp_gibbs_pg_stats",
    "nngp_binomial_newton_step_workspace_bytes",
    "nngp_binomial_newton_step",
    "nngp_binomial_check_partials",
    "nngp_logistic_normal",
    "nngp_factor_levels",
    "nngp_factor_launch_counts",
    "nngp_factor_solve_batch",
    "nngp_factor_cov_apply_batch",
    "nngp_factor_prior_draw_batch",
    "nngp_whiten_gram_workspace_bytes",
    "nngp_whiten_gram",
    "nngp_order_maxmin_workspace_bytes",
    "nngp_order_maxmin",
)

KIND_CODES = {"exponential": 0, "matern32": 1, "matern52": 2, "gaussian": 3, "spherical": 4, "matern": 5}
MATERN_NU_MAX = 50.0
ALGO_CODES = {"auto": 0, "lane": 1, "wave": 2, "quad": 4, "pairb": 5}
MAX_M = 63
MAX_DIM = 3
ND_MIN_DIM = 4   # the n-dimensional path (nngp_*_nd): MAX_DIM < dim <= ND_MAX_DIM
ND_MAX_DIM = 16  # NNGP_ND_MAX_DIM
ND_KINDS = ("exponential", "matern32", "matern52", "gaussian")
ABI_VERSION = 4  # NNGP_ABI_VERSION of include/nngp.h this binding's signatures follow
PLAN_INFO_LEN = 10  # NNGP_PLAN_INFO_LEN
CERT_INFO_LEN = 16  # NNGP_CERT_INFO_LEN
BLOCKS_MAX_M = 32  # nngp_bf_sweep_blocks: 1 <= m <= 32
LATENT_MAX_RHS = 8  # NNGP_LATENT_MAX_RHS: right-hand sides per batched latent call
PG_MAX_TRIALS = 1024  # NNGP_PG_MAX_TRIALS: binomial trials per location of a Polya-Gamma draw
WHITEN_MAX_COLS = 16  # NNGP_WHITEN_MAX_COLS: columns per nngp_whiten_gram call
FACTOR_MAX_FUSE_WIDTH = 1024  # NNGP_FACTOR_MAX_FUSE_WIDTH: rows per level the factor solve's narrow-run kernel takes


class NNGPExtensionError(RuntimeError):
    """The native library is missing, failed to load, or returned an error."""


_lib = None


def load() -> ctypes.CDLL:
    """Load (once) and return the native library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NNGPExtensionError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C pynngp_amd/csrc` (pynngp_amd has no CPU fallback)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    P, I32, I64, D, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t
    lib.nngp_version.restype = ctypes.c_char_p
    lib.nngp_abi_version.restype = I32
    if lib.nngp_abi_version() != ABI_VERSION:
        raise NNGPExtensionError(f"{LIB_PATH} has C ABI revision {lib.nngp_abi_version()}, this binding needs "
                                 f"{ABI_VERSION}: rebuild the library")
    lib.nngp_last_error.restype = ctypes.c_char_p
    lib.nngp_knn_workspace_bytes.argtypes = [I64, I32, I32]
    lib.nngp_knn_workspace_bytes.restype = SZ
    lib.nngp_knn_prior.argtypes = [P, I64, I32, I32, I64, I64, P, P, SZ, P]
    lib.nngp_knn_prior.restype = ctypes.c_int
    lib.nngp_knn_prior_rows.argtypes = [P, I64, I32, I32, P, I64, P, P, SZ, P]
    lib.nngp_knn_prior_rows.restype = ctypes.c_int
    lib.nngp_knn_query.argtypes = [P, I64, I32, P, I64, I32, P, P, SZ, P]
    lib.nngp_knn_query.restype = ctypes.c_int
    lib.nngp_bf_sweep_workspace_bytes.argtypes = [I64, I32, I32, I32, I32]
    lib.nngp_bf_sweep_workspace_bytes.restype = SZ
    lib.nngp_bf_sweep.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, D, D, D, P, P, P, P, P, P, SZ, I32, P]
    lib.nngp_bf_grad_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_bf_grad_workspace_bytes.restype = SZ
    lib.nngp_bf_grad.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, D, D, P, P, P, P, P, SZ, P]
    lib.nngp_bf_grad.restype = ctypes.c_int
    lib.nngp_bf_sweep_noise_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_bf_sweep_noise_workspace_bytes.restype = SZ
    lib.nngp_bf_sweep_noise.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, D, D, P, P, P, P, P, P, P, SZ, P]
    lib.nngp_bf_sweep_noise.restype = ctypes.c_int
    lib.nngp_bf_cross_noise.argtypes = [P, I64, I32, P, I64, P, P, I64, I32, I64, I32, D, D, D, P, P, P, P, P, P, P, P, P,
                                        SZ, P]
    lib.nngp_bf_cross_noise.restype = ctypes.c_int
    lib.nngp_bf_grad_noise.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, D, D, P, P, P, P, P, P, SZ, P]
    lib.nngp_bf_grad_noise.restype = ctypes.c_int
    lib.nngp_bf_sweep_sep_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_bf_sweep_sep_workspace_bytes.restype = SZ
    lib.nngp_bf_sweep_sep.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, I32, D, D, D, D, P, P, P, P, P, P, SZ, P]
    lib.nngp_bf_sweep_sep.restype = ctypes.c_int
    lib.nngp_bf_cross_sep.argtypes = [P, I64, I32, P, I64, P, P, I64, I32, I64, I32, I32, D, D, D, D, P, P, P, P, P, P, P,
                                      SZ, P]
    lib.nngp_bf_cross_sep.restype = ctypes.c_int
    lib.nngp_bf_grad_sep.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, I32, D, D, D, D, P, P, P, P, P, SZ, P]
    lib.nngp_bf_grad_sep.restype = ctypes.c_int
    lib.nngp_knn_nd_workspace_bytes.argtypes = [I64, I32, I32]
    lib.nngp_knn_nd_workspace_bytes.restype = SZ
    lib.nngp_knn_prior_nd.argtypes = [P, I64, I32, I32, I64, I64, P, P, SZ, P]
    lib.nngp_knn_prior_nd.restype = ctypes.c_int
    lib.nngp_knn_query_nd.argtypes = [P, I64, I32, P, I64, I32, P, P, SZ, P]
    lib.nngp_knn_query_nd.restype = ctypes.c_int
    lib.nngp_bf_sweep_nd_workspace_bytes.argtypes = [I64, I32, I32]
    lib.nngp_bf_sweep_nd_workspace_bytes.restype = SZ
    lib.nngp_bf_sweep_nd.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, P, D, P, P, P, P, P, P, SZ, P]
    lib.nngp_bf_sweep_nd.restype = ctypes.c_int
    lib.nngp_bf_cross_nd.argtypes = [P, I64, I32, P, I64, P, P, I64, I32, I64, I32, D, P, D, P, P, P, P, P, P, P, SZ, P]
    lib.nngp_bf_cross_nd.restype = ctypes.c_int
    lib.nngp_bf_grad_nd.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, P, D, P, P, P, P, P, SZ, P]
    lib.nngp_bf_grad_nd.restype = ctypes.c_int
    lib.nngp_bf_grad_aniso_workspace_bytes.argtypes = [I64, I32, I32]
    lib.nngp_bf_grad_aniso_workspace_bytes.restype = SZ
    lib.nngp_bf_grad_aniso.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, P, D, P, P, P, P, P, SZ, P]
    lib.nngp_bf_grad_aniso.restype = ctypes.c_int
    lib.nngp_bf_grad_matern_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_bf_grad_matern_workspace_bytes.restype = SZ
    lib.nngp_bf_grad_matern.argtypes = [P, I64, I32, P, P, I64, I32, I64, D, D, D, D, P, P, P, P, P, SZ, P]
    lib.nngp_bf_grad_matern.restype = ctypes.c_int
    lib.nngp_matern_eval_d.argtypes = [P, I64, D, P, P, P]
    lib.nngp_matern_eval_d.restype = ctypes.c_int
    lib.nngp_bf_dphi_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_bf_dphi_workspace_bytes.restype = SZ
    lib.nngp_bf_dphi.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, D, D, P, P, P, P, P, P, SZ, P]
    lib.nngp_bf_dphi.restype = ctypes.c_int
    lib.nngp_bf_fisher_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_bf_fisher_workspace_bytes.restype = SZ
    lib.nngp_bf_fisher.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, D, D, P, P, P, P, P, P, P, SZ, P]
    lib.nngp_bf_fisher.restype = ctypes.c_int
    lib.nngp_bf_cross.argtypes = [P, I64, I32, P, I64, P, P, I64, I32, I64, I32, D, D, D, D, P, P, P, P, P, P, P, SZ,
                                  I32, P]
    lib.nngp_bf_cross.restype = ctypes.c_int
    lib.nngp_row_order_workspace_bytes.argtypes = [I64]
    lib.nngp_row_order_workspace_bytes.restype = SZ
    lib.nngp_row_order.argtypes = [P, I64, I32, P, I32, I64, I64, P, P, P, SZ, P]
    lib.nngp_row_order.restype = ctypes.c_int
    lib.nngp_combine_partials.argtypes = [P, I32, P, P]
    lib.nngp_combine_partials_batch.argtypes = [P, I32, I64, P, P]
    lib.nngp_matern_eval.argtypes = [P, I64, D, P, P]
    lib.nngp_matern_eval.restype = ctypes.c_int
    lib.nngp_joint_entries.argtypes = [I32]
    lib.nngp_joint_entries.restype = I64
    lib.nngp_joint_dist.argtypes = [P, I64, I32, P, I64, P, P, I64, I32, I64, P, P]
    lib.nngp_joint_dist.restype = ctypes.c_int
    lib.nngp_bf_sweep_blocks_workspace_bytes.argtypes = [I64]
    lib.nngp_bf_sweep_blocks_workspace_bytes.restype = SZ
    lib.nngp_bf_sweep_blocks.argtypes = [P, P, P, I64, I64, I32, I64, I64, P, P, P, P, P, P, P, SZ, P]
    lib.nngp_bf_sweep_blocks.restype = ctypes.c_int
    lib.nngp_combine_partials_batch.restype = ctypes.c_int
    lib.nngp_bf_finalize.argtypes = [P, ctypes.c_size_t, I64, I32, I32, I32, I32, P, P]
    lib.nngp_bf_finalize.restype = ctypes.c_int
    lib.nngp_resolve_algo.argtypes = [I32, I32, I32, I32]
    lib.nngp_resolve_algo.restype = I32
    lib.nngp_resolve_algo_nu.argtypes = [I32, I32, I32, I32, D]
    lib.nngp_resolve_algo_nu.restype = I32
    lib.nngp_combine_partials.restype = ctypes.c_int
    U64 = ctypes.c_uint64
    lib.nngp_reverse_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_reverse_workspace_bytes.restype = SZ
    lib.nngp_reverse_neighbors.argtypes = [P, I64, I32, P, P, P, P, SZ, P]
    lib.nngp_reverse_neighbors.restype = ctypes.c_int
    lib.nngp_color_moral_graph.argtypes = [P, P, P, I64, I32, P]
    lib.nngp_color_moral_graph.restype = I64
    lib.nngp_gibbs_prep_bytes.argtypes = [I64, I32]
    lib.nngp_gibbs_prep_bytes.restype = SZ
    lib.nngp_gibbs_prepare.argtypes = [P, P, P, P, P, P, I64, I32, P, SZ, P]
    lib.nngp_gibbs_prepare.restype = ctypes.c_int
    lib.nngp_gibbs_member_rows.argtypes = [P, I64, P, P, P]
    lib.nngp_gibbs_member_rows.restype = ctypes.c_int
    lib.nngp_gibbs_w_sweep.argtypes = [P, P, I32, P, I64, I32, D, D, P, P, P, P, P, P, U64, U64, P]
    lib.nngp_gibbs_w_sweep.restype = ctypes.c_int
    lib.nngp_gibbs_normals.argtypes = [I64, U64, U64, P, P]
    lib.nngp_gibbs_normals.restype = ctypes.c_int
    lib.nngp_gibbs_prepare_range.argtypes = [P, P, P, P, P, I64, I32, I64, I64, P, SZ, P]
    lib.nngp_gibbs_prepare_range.restype = ctypes.c_int
    lib.nngp_gibbs_w_color.argtypes = [P, I64, P, I64, I32, D, D, P, P, P, P, P, P, U64, U64, P, P]
    lib.nngp_gibbs_w_color.restype = ctypes.c_int
    lib.nngp_gibbs_w_color_dev.argtypes = [P, I64, P, I64, I32, P, P, P, P, P, P, P, P, P]
    lib.nngp_gibbs_w_color_dev.restype = ctypes.c_int
    lib.nngp_gibbs_w_apply.argtypes = [P, I64, P, P, I64, I32, P, P, P, P, P]
    lib.nngp_gibbs_w_apply.restype = ctypes.c_int
    lib.nngp_gibbs_stats_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_gibbs_stats_workspace_bytes.restype = SZ
    lib.nngp_gibbs_stats.argtypes = [I64, P, P, P, P, P, I32, P, P, P, P, SZ, P]
    lib.nngp_gibbs_stats.restype = ctypes.c_int
    lib.nngp_polya_gamma.argtypes = [I64, P, P, U64, U64, P, P, P]
    lib.nngp_polya_gamma.restype = ctypes.c_int
    lib.nngp_gibbs_pg_update.argtypes = [I64, P, P, P, P, U64, U64, P, P, P, P]
    lib.nngp_gibbs_pg_update.restype = ctypes.c_int
    lib.nngp_gibbs_pg_stats_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_gibbs_pg_stats_workspace_bytes.restype = SZ
    lib.nngp_gibbs_pg_stats.argtypes = [I64, P, P, P, P, P, I32, P, P, P, P]
    lib.nngp_gibbs_pg_stats.restype = ctypes.c_int
    lib.nngp_binomial_newton_step_workspace_bytes.argtypes = [I64]
    lib.nngp_binomial_newton_step_workspace_bytes.restype = SZ
    lib.nngp_binomial_newton_step.argtypes = [I64, P, P, P, P, P, P, P, P, P, SZ, P]
    lib.nngp_binomial_newton_step.restype = ctypes.c_int
    lib.nngp_binomial_check_partials.argtypes = [P, P, P]
    lib.nngp_binomial_check_partials.restype = ctypes.c_int
    lib.nngp_logistic_normal.argtypes = [I64, P, P, P, P]
    lib.nngp_logistic_normal.restype = ctypes.c_int
    lib.nngp_bf_sweep.restype = ctypes.c_int
    lib.nngp_color_moral_graph_dev.argtypes = [P, P, P, I64, I32, P, P, SZ, P]
    lib.nngp_color_moral_graph_dev.restype = I64
    lib.nngp_gibbs_w_sweep_tiles.argtypes = [P, P, P, I32, P, P, I32, P, P, P, P, I64, I32, I64, D, D, P, P, P, P,
                                             P, P]
    lib.nngp_gibbs_w_sweep_tiles.restype = ctypes.c_int
    lib.nngp_gibbs_w_sweep_chains.argtypes = [P, P, I32, I32, P, I64, I32, P, P, P, P, P, P, P, P, P]
    lib.nngp_gibbs_w_sweep_chains.restype = ctypes.c_int
    lib.nngp_gibbs_w_sweep_chains_il.argtypes = [P, P, I32, I32, P, I64, I32, P, P, P, P, P, P, P, P, P]
    lib.nngp_gibbs_w_sweep_chains_il.restype = ctypes.c_int
    lib.nngp_pair_plan_supported.argtypes = [I32, I32, I32]
    lib.nngp_pair_plan_supported.restype = ctypes.c_int
    lib.nngp_pair_plan_bytes.argtypes = [I64, I32, I32]
    lib.nngp_pair_plan_bytes.restype = SZ
    lib.nngp_pair_plan_build.argtypes = [P, P, I64, I32, I64, I64, I32, P, SZ, P, P]
    lib.nngp_pair_plan_build.restype = ctypes.c_int
    lib.nngp_bf_sweep_plan.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, D, D, P, P, P, P, P, P, SZ, P, SZ, P,
                                       P]
    lib.nngp_bf_sweep_plan.restype = ctypes.c_int
    lib.nngp_nbr_cert_bytes.argtypes = [I64]
    lib.nngp_nbr_cert_bytes.restype = SZ
    lib.nngp_nbr_cert_build.argtypes = [P, I64, I32, P, P, I64, I32, I64, P, SZ, P, P]
    lib.nngp_nbr_cert_build.restype = ctypes.c_int
    lib.nngp_nbr_cert_trusted_tiles.argtypes = [P, I32, D, D, D]
    lib.nngp_nbr_cert_trusted_tiles.restype = I64
    lib.nngp_bf_sweep_cert.argtypes = [P, I64, I32, P, P, I64, I32, I64, I32, D, D, D, D, P, P, P, P, P, P, SZ, I32, P,
                                       SZ, P, P]
    lib.nngp_bf_sweep_cert.restype = ctypes.c_int
    lib.nngp_precision_workspace_bytes.argtypes = [I64]
    lib.nngp_precision_workspace_bytes.restype = SZ
    lib.nngp_precision_apply.argtypes = [P, P, P, P, P, P, I64, I32, D, P, P, P, P, SZ, P]
    lib.nngp_precision_apply.restype = ctypes.c_int
    lib.nngp_precision_sqrt_t_apply.argtypes = [P, P, P, P, P, P, I64, I32, D, P, P, P, P, P, SZ, P]
    lib.nngp_precision_sqrt_t_apply.restype = ctypes.c_int
    lib.nngp_latent_cg_workspace_bytes.argtypes = [I64]
    lib.nngp_latent_cg_workspace_bytes.restype = SZ
    lib.nngp_latent_cg.argtypes = [P, P, P, P, P, P, I64, I32, D, P, P, P, D, I64, I32, P, P, SZ, P]
    lib.nngp_latent_cg.restype = ctypes.c_int
    lib.nngp_precision_batch_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_precision_batch_workspace_bytes.restype = SZ
    lib.nngp_precision_apply_batch.argtypes = [P, P, P, P, P, P, I64, I32, D, P, I32, P, P, P, SZ, P]
    lib.nngp_precision_apply_batch.restype = ctypes.c_int
    lib.nngp_precision_sqrt_t_apply_batch.argtypes = [P, P, P, P, P, P, I64, I32, D, P, I32, P, P, P, P, SZ, P]
    lib.nngp_precision_sqrt_t_apply_batch.restype = ctypes.c_int
    lib.nngp_latent_cg_batch_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_latent_cg_batch_workspace_bytes.restype = SZ
    lib.nngp_latent_cg_batch.argtypes = [P, P, P, P, P, P, I64, I32, D, P, I32, P, P, D, I64, I32, P, P, SZ, P]
    lib.nngp_latent_cg_batch.restype = ctypes.c_int
    lib.nngp_precision_diag.argtypes = [P, I64, I32, D, P, P, P]
    lib.nngp_precision_diag.restype = ctypes.c_int
    lib.nngp_precision_ref_batch_workspace_bytes.argtypes = [I64, I64, I32]
    lib.nngp_precision_ref_batch_workspace_bytes.restype = SZ
    lib.nngp_precision_ref_apply_batch.argtypes = [P, P, P, P, P, P, I64, I64, I32, D, P, I32, P, P, P, SZ, P]
    lib.nngp_precision_ref_apply_batch.restype = ctypes.c_int
    lib.nngp_precision_ref_sqrt_t_apply_batch.argtypes = [P, P, P, P, P, P, I64, I64, I32, D, P, I32, P, P, P, P, SZ,
                                                          P]
    lib.nngp_precision_ref_sqrt_t_apply_batch.restype = ctypes.c_int
    lib.nngp_precision_ref_fold_batch.argtypes = [P, P, P, P, P, P, I64, I64, I32, D, P, I32, P, P, P, SZ, P]
    lib.nngp_precision_ref_fold_batch.restype = ctypes.c_int
    lib.nngp_precision_ref_diag.argtypes = [P, P, P, P, P, P, I64, I64, I32, D, P, P, P, SZ, P]
    lib.nngp_precision_ref_diag.restype = ctypes.c_int
    lib.nngp_latent_ref_cg_batch_workspace_bytes.argtypes = [I64, I64, I32]
    lib.nngp_latent_ref_cg_batch_workspace_bytes.restype = SZ
    lib.nngp_latent_ref_cg_batch.argtypes = [P, P, P, P, P, P, I64, I64, I32, D, P, I32, P, P, D, I64, I32, P, P, SZ,
                                             P]
    lib.nngp_latent_ref_cg_batch.restype = ctypes.c_int
    lib.nngp_latent_ref_cg_batch_trace.argtypes = [P, P, P, P, P, P, I64, I64, I32, D, P, I32, P, P, D, I64, I32, P, P,
                                                   SZ, P, I64, P]
    lib.nngp_latent_ref_cg_batch_trace.restype = ctypes.c_int
    lib.nngp_latent_ref_leaves_batch.argtypes = [P, P, P, P, P, P, I64, I64, I32, D, P, I32, P, P, P, P, P]
    lib.nngp_latent_ref_leaves_batch.restype = ctypes.c_int
    lib.nngp_latent_rows_dot2_batch.argtypes = [P, P, P, I64, I64, I32, I32, P, P, P, P]
    lib.nngp_latent_rows_dot2_batch.restype = ctypes.c_int
    lib.nngp_factor_levels.argtypes = [P, I64, I32, I32, P, P, P, P]
    lib.nngp_factor_levels.restype = ctypes.c_int
    lib.nngp_factor_launch_counts.argtypes = [P, I64, I32, P, P]
    lib.nngp_factor_launch_counts.restype = ctypes.c_int
    lib.nngp_factor_solve_batch.argtypes = [P, P, P, P, P, P, P, P, P, I64, I64, I32, I32, I32, I32, P, P, P]
    lib.nngp_factor_solve_batch.restype = ctypes.c_int
    lib.nngp_factor_cov_apply_batch.argtypes = [P, P, P, P, P, P, P, P, P, P, I64, P, P, P, I64, I64, I32, D, I32, I32,
                                                P, P, P]
    lib.nngp_factor_cov_apply_batch.restype = ctypes.c_int
    lib.nngp_factor_prior_draw_batch.argtypes = [P, P, P, P, P, P, I64, I64, I32, D, I32, I32, P, U64, U64, P, P]
    lib.nngp_factor_prior_draw_batch.restype = ctypes.c_int
    lib.nngp_whiten_gram_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_whiten_gram_workspace_bytes.restype = SZ
    lib.nngp_whiten_gram.argtypes = [P, P, P, P, I64, I32, I64, I64, I32, P, P, P, P, P, SZ, P]
    lib.nngp_whiten_gram.restype = ctypes.c_int
    lib.nngp_order_maxmin_workspace_bytes.argtypes = [I64, I32]
    lib.nngp_order_maxmin_workspace_bytes.restype = SZ
    lib.nngp_order_maxmin.argtypes = [P, I64, I32, ctypes.c_uint32, P, P, P, SZ, P]
    lib.nngp_order_maxmin.restype = ctypes.c_int
    lib.nngp_check_partials.argtypes = [P, P, P]
    lib.nngp_check_partials.restype = ctypes.c_int
    lib.nngp_loglik_from_partials.argtypes = [P, I64]
    lib.nngp_loglik_from_partials.restype = D
    _lib = lib
    return lib


def version() -> str:
    return load().nngp_version().decode()


def resolve_algo(algo: str, m: int, kind: str, dim: int, nu: Optional[float] = None) -> str:
    """The kernel ``algo`` ("auto" or explicit) runs as for (m, kind, dim) (nngp_resolve_algo; with ``nu``
    for the ``matern`` kind, whose pair-kernel table covers nu >= ~0.45: nngp_resolve_algo_nu)."""
    if nu is not None:
        code = load().nngp_resolve_algo_nu(ALGO_CODES[algo], int(m), KIND_CODES[kind], int(dim), float(nu))
    else:
        code = load().nngp_resolve_algo(ALGO_CODES[algo], int(m), KIND_CODES[kind], int(dim))
    names = {v: k for k, v in ALGO_CODES.items()}
    return names.get(code, str(code))


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().nngp_last_error().decode()
        raise NNGPExtensionError(f"{what} failed ({rc}): {msg}")


def _require_gpu(*tensors: Optional[torch.Tensor]) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise NNGPExtensionError(
                f"pynngp_amd needs ROCm GPU tensors (got {t.device}); there is no CPU fallback"
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise NNGPExtensionError(f"tensors on different devices: {dev} vs {t.device}")
    if dev is None:
        raise NNGPExtensionError("no tensor arguments")
    return dev


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _workspace(nbytes: int, dev: torch.device) -> torch.Tensor:
    # torch's caching allocator returns >= 512-byte aligned blocks; the first 256 bytes (the pair kernel's
    # header: tile count and the fused fold's ticket) start at zero, as include/nngp.h requires
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    ws[:256].zero_()
    return ws


def _as_coords(coords: torch.Tensor) -> torch.Tensor:
    """float64 (N, dim) ordinates, 1 <= dim <= 3 (nngp.py:55-61 takes any dimension)."""
    if coords.dim() != 2 or not 1 <= coords.shape[1] <= MAX_DIM or coords.dtype != torch.float64:
        raise ValueError(f"coords must be float64 (N, dim), 1 <= dim <= {MAX_DIM}, got {tuple(coords.shape)} "
                         f"{coords.dtype}")
    return coords.contiguous()


def _same_dim(*coords: torch.Tensor) -> int:
    dims = {c.shape[1] for c in coords}
    if len(dims) != 1:
        raise ValueError(f"coordinate arrays of different dimensions: {sorted(dims)}")
    return dims.pop()


def _check_out(t: Optional[torch.Tensor], name: str, shape, dev: torch.device) -> None:
    """Caller-supplied output buffer: float64, the exact shape, contiguous, on dev (the
    kernel writes through the raw pointer, so a wrong buffer would be written out of bounds)."""
    if t is None:
        return
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise ValueError(f"{name} must be a contiguous float64 {tuple(shape)} tensor on {dev}, got "
                         f"{t.dtype} {tuple(t.shape)} contiguous={t.is_contiguous()} on {t.device}")


def knn_prior(coords: torch.Tensor, m: int, q0: int = 0, q1: Optional[int] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Ordered prior neighbour sets for rows [q0, q1): int32 (q1-q0, m), -1 padded.

    Replaces ``NNGP._make_s_neighbor_sets`` (pyNNGP/nngp.py:49-62).
    """
    coords = _as_coords(coords)
    dev = _require_gpu(coords)
    n = coords.shape[0]
    q1 = n if q1 is None else int(q1)
    if not 0 <= q0 <= q1 <= n:
        raise ValueError(f"query rows [{q0}, {q1}) outside [0, {n})")
    if out is None:
        out = torch.empty((q1 - q0, m), dtype=torch.int32, device=dev)
    lib = load()
    d = coords.shape[1]
    ws = _workspace(lib.nngp_knn_workspace_bytes(n, d, m), dev)
    _check(lib.nngp_knn_prior(_ptr(coords), n, d, m, q0, q1, _ptr(out), _ptr(ws), ws.numel(), _stream(dev)),
           "nngp_knn_prior")
    return out


def knn_prior_rows(coords: torch.Tensor, m: int, rows: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Prior neighbour sets of the locations ``rows`` (int32 point indices, any order):
    row t of the result is the set of point ``rows[t]`` (nngp_knn_prior_rows)."""
    coords = _as_coords(coords)
    if rows.dtype != torch.int32 or rows.dim() != 1:
        raise ValueError("rows must be int32 (n_rows,)")
    rows = rows.contiguous()
    dev = _require_gpu(coords, rows)
    n = coords.shape[0]
    if out is None:
        out = torch.empty((rows.shape[0], m), dtype=torch.int32, device=dev)
    lib = load()
    d = coords.shape[1]
    ws = _workspace(lib.nngp_knn_workspace_bytes(n, d, m), dev)
    _check(lib.nngp_knn_prior_rows(_ptr(coords), n, d, m, _ptr(rows), rows.shape[0], _ptr(out), _ptr(ws), ws.numel(),
                                   _stream(dev)), "nngp_knn_prior_rows")
    return out


def knn_query(ref: torch.Tensor, query: torch.Tensor, k: int) -> torch.Tensor:
    """k nearest reference points of every query point (no prior restriction).

    int32 (n_query, k) in (rdist, index) order; -1 padded when k > n_ref.  Used for
    ``_init_ws`` (pyNNGP/nngp.py:45-47, sklearn KNeighborsRegressor(5)) and the
    off-reference sets of ``_make_t_neighbor_sets`` (nngp.py:64-71).
    """
    ref = _as_coords(ref)
    query = _as_coords(query)
    d = _same_dim(ref, query)
    dev = _require_gpu(ref, query)
    out = torch.empty((query.shape[0], k), dtype=torch.int32, device=dev)
    lib = load()
    ws = _workspace(lib.nngp_knn_workspace_bytes(ref.shape[0], d, k), dev)
    _check(lib.nngp_knn_query(_ptr(ref), ref.shape[0], d, _ptr(query), query.shape[0], k, _ptr(out), _ptr(ws),
                              ws.numel(), _stream(dev)), "nngp_knn_query")
    return out


def _check_kind(kind: str, nu: Optional[float]) -> float:
    """The kind's code must exist; the ``matern`` kind needs 0 < nu <= 50 (returned as the C argument)."""
    if kind not in KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}; expected one of {sorted(KIND_CODES)}")
    if kind == "matern":
        if nu is None or not 0.0 < float(nu) <= MATERN_NU_MAX:
            raise ValueError(f"the matern kind needs a smoothness 0 < nu <= {MATERN_NU_MAX:g} (got {nu!r})")
        return float(nu)
    return -1.0


class PairPlan:
    """A wave pair plan (``nngp_pair_plan_build``, include/nngp.h): the distinct covariance pairs of
    every sweep wavefront and each lane's map into them, for one (nbr, order, i0, n_points).  Passed to
    :func:`bf_sweep` (``plan=``), it evaluates each shared covariance once per wave; B / F / R and the
    partials are bit-identical to the unplanned pair kernel's.  The plan is stale once nbr or order
    change (rebuild it, as the neighbour sets themselves): :meth:`matches` compares the buffers and
    torch's in-place version counters, the C ABI the buffers, the kernel a per-location checksum."""

    def __init__(self, buf: torch.Tensor, info, nbr: torch.Tensor, order: Optional[torch.Tensor]):
        self.buf = buf
        self.info = (ctypes.c_int64 * PLAN_INFO_LEN)(*info)
        self.n_planned, self.n_direct = int(info[0]), int(info[1])
        self.n_rows, self.m, self.dim, self.i0, self.n_points = (int(v) for v in info[2:7])
        self._nbr_ptr, self._order_ptr = nbr.data_ptr(), (order.data_ptr() if order is not None else 0)
        self._versions = (nbr._version, order._version if order is not None else 0)

    def matches(self, nbr: torch.Tensor, order: Optional[torch.Tensor], i0: int, n_points: int, dim: int) -> bool:
        """True when this plan was built for these nbr / order tensors (same storage, not modified in place
        since) and this geometry."""
        return (nbr.data_ptr() == self._nbr_ptr and (order.data_ptr() if order is not None else 0) == self._order_ptr
                and (nbr._version, order._version if order is not None else 0) == self._versions
                and tuple(nbr.shape) == (self.n_rows, self.m) and i0 == self.i0 and n_points == self.n_points
                and dim == self.dim)


def pair_plan_read_bytes(buf: torch.Tensor, m: int) -> int:
    """Bytes a planned sweep streams from its plan (pair_plan.h: per planned wave the three header words,
    the map chunks, the checksums, the U list and the pair words, in whole rounds) -- the plan's share of
    the sweep's input traffic.  Reads the wave headers back (a setup-time helper: one synchronisation)."""
    hdr = buf[:256].view(torch.int64).cpu()
    nreg, sb = int(hdr[6]), int(hdr[9])
    if nreg == 0:
        return 0
    wsb = sb // 4
    w = buf[256:256 + nreg * sb].view(nreg * 4, wsb)[:, :12].contiguous().view(torch.int32).long().cpu()
    nU, nE, st = w[:, 0], w[:, 1].clamp(min=0), w[:, 2]
    planned = (st.view(nreg, 4) == 0).all(1).repeat_interleave(4)
    np_ = (m + 2) // 2
    che = (np_ * np_ + 7) // 8
    per = 12 + che * 1024 + 256 + 256 * ((nU + 63) // 64) + 1024 * ((nE + 255) // 256)
    return int(per[planned].sum())


def pair_plan_supported(m: int, kind: str, dim: int) -> bool:
    """Whether wave pair plans serve (m, kind, dim) (2 <= m <= 17, kinds exponential .. spherical, dim 1..3)."""
    return kind in KIND_CODES and bool(load().nngp_pair_plan_supported(int(m), KIND_CODES[kind], int(dim)))


def pair_plan(nbr: torch.Tensor, n_points: int, dim: int, i0: int = 0,
              order: Optional[torch.Tensor] = None) -> PairPlan:
    """Build the wave pair plan of a sweep over ``nbr`` (int32 (rows, m) on the GPU; rows are locations
    ``i0 + (order[t] if order else t)`` of an ``n_points``-point field of dimension ``dim``).  A setup
    call: it synchronises torch's current stream once (the plan's tile counts come back to the host)."""
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    dev = _require_gpu(nbr, order)
    rows, m = nbr.shape
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    lib = load()
    nbytes = lib.nngp_pair_plan_bytes(rows, m, dim)
    if nbytes == 0:
        raise NNGPExtensionError(f"no pair plans for m={m}, dim={dim} (2 <= m <= 17, dim 1..3)")
    buf = _workspace(nbytes, dev)
    info = (ctypes.c_int64 * PLAN_INFO_LEN)()
    _check(lib.nngp_pair_plan_build(_ptr(nbr), _ptr(order), rows, m, int(i0), int(n_points), int(dim), _ptr(buf),
                                    buf.numel(), info, _stream(dev)), "nngp_pair_plan_build")
    return PairPlan(buf, list(info), nbr, order)


def bf_sweep(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind: str, sigma2: float, phi: float,
             tau2: float = 0.0, values: Optional[torch.Tensor] = None, want_bf: bool = True,
             algo: str = "auto", B: Optional[torch.Tensor] = None, F: Optional[torch.Tensor] = None,
             partials: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
             order: Optional[torch.Tensor] = None,
             R: Optional[torch.Tensor] = None,
             defer: bool = False, nu: Optional[float] = None, plan: Optional[PairPlan] = None,
             cert=None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], torch.Tensor]:
    """Fused B/F + log-likelihood sweep over rows ``i0 .. i0 + len(nbr)``.

    ``cert``: ``(buffer, info)`` of :func:`nbr_cert` for exactly these coords / nbr / order tensors and i0
    (nngp_bf_sweep_cert: the same bits; tiles without padding or bad indices skip the index checks and clamps).

    ``plan``: a :func:`pair_plan` of this nbr / order / i0 (the pair kernel with every shared
    covariance evaluated once per tile; kinds exponential .. spherical, algo ``auto`` / ``pairb``).

    ``nu``: the smoothness of the ``matern`` kind (0 < nu <= 50; required there, ignored otherwise).

    ``defer=True`` (needs ``workspace``): the final fold is left to :func:`bf_finalize`
    on the same workspace (e.g. on another stream); partials is returned as None.

    Returns ``(B, F, partials)`` (B, F None when ``want_bf`` is False); partials is a
    float64 device tensor ``[sum log F, sum r^2/F, first bad-pivot row, first bad-index row]``.
    Stream-ordered on torch's current stream; no host synchronisation.  With
    ``order`` (int32 (rows,), from :func:`row_order`) row t of ``nbr`` must hold the
    neighbours of location ``i0 + order[t]`` (pass ``nbr_sorted``); only the visiting
    order changes, B and F are written at their natural rows.
    """
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    if values is not None:
        if values.dtype != torch.float64 or values.shape != (coords.shape[0],):
            raise ValueError("values must be float64 (N,)")
        values = values.contiguous()
    dev = _require_gpu(coords, nbr, values, order)
    rows, m = nbr.shape
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    nu = _check_kind(kind, nu)
    lib = load()
    a = ALGO_CODES[algo]
    if want_bf:
        _check_out(B, "B", (rows, m), dev)
        _check_out(F, "F", (rows,), dev)
        B = torch.empty((rows, m), dtype=torch.float64, device=dev) if B is None else B
        F = torch.empty((rows,), dtype=torch.float64, device=dev) if F is None else F
    else:
        B = F = None
    if defer:
        partials = None
    else:
        _check_out(partials, "partials", (4,), dev)
        partials = torch.empty(4, dtype=torch.float64, device=dev) if partials is None else partials
    d = coords.shape[1]
    need = lib.nngp_bf_sweep_workspace_bytes(rows, m, KIND_CODES[kind], d, a)
    if workspace is None or workspace.numel() < need:
        if defer:
            raise ValueError("defer=True needs a workspace of nngp_bf_sweep_workspace_bytes bytes")
        workspace = _workspace(need, dev)
    _check_out(R, "R", (rows,), dev)
    if workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous tensor on the sweep's device")
    if plan is not None:
        if algo not in ("auto", "pairb"):
            raise ValueError(f"a pair plan runs the pair kernel, not algo {algo!r}")
        if not isinstance(plan, PairPlan) or plan.buf.device != dev:
            raise ValueError("plan must be a PairPlan on the sweep's device")
        if not plan.matches(nbr, order, i0, coords.shape[0], d):
            raise ValueError("stale pair plan: it was built for other nbr / order tensors (or they were modified in "
                             "place since) or another geometry; rebuild it with pair_plan")
        _check(lib.nngp_bf_sweep_plan(_ptr(coords), coords.shape[0], d, _ptr(nbr), _ptr(order), rows, m, i0,
                                      KIND_CODES[kind], float(sigma2), float(phi), float(tau2), _ptr(values), _ptr(B),
                                      _ptr(F), _ptr(R), _ptr(partials), _ptr(workspace), workspace.numel(),
                                      _ptr(plan.buf), plan.buf.numel(), plan.info, _stream(dev)),
               "nngp_bf_sweep_plan")
        return B, F, partials
    if cert is not None:
        cbuf, cinfo = cert
        if cbuf.device != dev:
            raise ValueError("cert must be on the sweep's device")
        _check(lib.nngp_bf_sweep_cert(_ptr(coords), coords.shape[0], d, _ptr(nbr), _ptr(order), rows, m, i0,
                                      KIND_CODES[kind], float(sigma2), float(phi), float(tau2), nu, _ptr(values),
                                      _ptr(B), _ptr(F), _ptr(R), _ptr(partials), _ptr(workspace), workspace.numel(), a,
                                      _ptr(cbuf), cbuf.numel(), cinfo, _stream(dev)),
               "nngp_bf_sweep_cert")
        return B, F, partials
    _check(lib.nngp_bf_sweep(_ptr(coords), coords.shape[0], d, _ptr(nbr), _ptr(order), rows, m, i0, KIND_CODES[kind],
                             float(sigma2), float(phi), float(tau2), nu, _ptr(values), _ptr(B), _ptr(F), _ptr(R),
                             _ptr(partials), _ptr(workspace), workspace.numel(), a, _stream(dev)),
           "nngp_bf_sweep")
    return B, F, partials


GRAD_MAX_M = 32  # nngp_bf_grad: 1 <= m <= 32, kinds exponential .. spherical


def bf_grad(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind: str, sigma2: float, phi: float, tau2: float,
            values: torch.Tensor, want_rows: bool = False, order: Optional[torch.Tensor] = None,
            workspace: Optional[torch.Tensor] = None
            ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Analytic log-likelihood gradient sweep (``nngp_bf_grad``, include/nngp.h) over rows ``i0 .. i0 + len(nbr)``.

    Returns ``(partials, grad, G)``: the four partials of :func:`bf_sweep`, ``grad`` = the summed
    d loglik / d (sigma2, phi, tau2) (float64 (3,) device tensors, fixed fold order) and, with ``want_rows``,
    ``G`` (rows, 3), the per-location terms at their natural rows (NaN in rows flagged in partials[2]).
    Stream-ordered on torch's current stream; no host synchronisation.  Kinds exponential .. spherical,
    1 <= m <= 32; ``order`` as in :func:`bf_sweep`.
    """
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    if values is None or values.dtype != torch.float64 or values.shape != (coords.shape[0],):
        raise ValueError("values must be float64 (N,)")
    values = values.contiguous()
    rows, m = nbr.shape
    if kind not in KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind == "matern":
        raise NotImplementedError("the gradient sweep serves the kinds exponential .. spherical, not the general-nu "
                                  "matern kind")
    if not 1 <= m <= GRAD_MAX_M:
        raise NotImplementedError(f"the gradient sweep serves 1 <= m <= {GRAD_MAX_M} (m={m})")
    dev = _require_gpu(coords, nbr, values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    lib = load()
    need = lib.nngp_bf_grad_workspace_bytes(rows, m)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    if workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous tensor on the sweep's device")
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    grad = torch.empty(3, dtype=torch.float64, device=dev)
    G = torch.empty((rows, 3), dtype=torch.float64, device=dev) if want_rows else None
    _check(lib.nngp_bf_grad(_ptr(coords), coords.shape[0], coords.shape[1], _ptr(nbr), _ptr(order), rows, m, i0,
                            KIND_CODES[kind], float(sigma2), float(phi), float(tau2), _ptr(values), _ptr(G),
                            _ptr(partials), _ptr(grad), _ptr(workspace), workspace.numel(), _stream(dev)),
           "nngp_bf_grad")
    return partials, grad, G


def _phi_vec(phi_vec, dim: int) -> Tuple[float, ...]:
    """The per-axis decays as ``dim`` positive finite floats."""
    try:
        phi = tuple(float(p) for p in phi_vec)
    except TypeError:
        raise ValueError("phi_vec must be a sequence of dim positive floats") from None
    if len(phi) != dim:
        raise ValueError(f"phi_vec has {len(phi)} entries for {dim}-dimensional coordinates")
    if not all(p > 0.0 and np.isfinite(p) for p in phi):
        raise ValueError(f"every phi_k must be positive and finite, got {phi}")
    return phi


def bf_grad_aniso(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind: str, sigma2: float, phi_vec, tau2: float,
                  values: torch.Tensor, order: Optional[torch.Tensor] = None, want_rows: bool = False,
                  workspace: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Per-axis gradient sweep (``nngp_bf_grad_aniso``, include/nngp.h) over rows ``i0 .. i0 + len(nbr)``, for the
    covariance with one decay per axis, u = sqrt(sum_k (phi_k (a_k - b_k))^2).  ``coords`` are the raw coordinates;
    ``phi_vec`` has one entry per column.

    Returns ``(partials, grad, G)``: the four partials of :func:`bf_sweep` (at phi = 1 on the scaled coordinates),
    ``grad`` = the summed d loglik / d (sigma2, phi_1 .. phi_dim, tau2) (float64 (dim + 2,), fixed fold order) and,
    with ``want_rows``, ``G`` (rows, dim + 2) (NaN in rows flagged in partials[2]).  Stream-ordered on torch's
    current stream; no host synchronisation.  Kinds exponential .. spherical, 1 <= m <= 32.
    """
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    if values is None or values.dtype != torch.float64 or values.shape != (coords.shape[0],):
        raise ValueError("values must be float64 (N,)")
    values = values.contiguous()
    rows, m = nbr.shape
    dim = coords.shape[1]
    if kind not in KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind == "matern":
        raise NotImplementedError("the per-axis gradient sweep serves the kinds exponential .. spherical, not the "
                                  "general-nu matern kind")
    if not 1 <= m <= GRAD_MAX_M:
        raise NotImplementedError(f"the per-axis gradient sweep serves 1 <= m <= {GRAD_MAX_M} (m={m})")
    phi = _phi_vec(phi_vec, dim)
    dev = _require_gpu(coords, nbr, values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    lib = load()
    need = lib.nngp_bf_grad_aniso_workspace_bytes(rows, m, dim)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    if workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous tensor on the sweep's device")
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    grad = torch.empty(dim + 2, dtype=torch.float64, device=dev)
    G = torch.empty((rows, dim + 2), dtype=torch.float64, device=dev) if want_rows else None
    phi_host = (ctypes.c_double * dim)(*phi)
    _check(lib.nngp_bf_grad_aniso(_ptr(coords), coords.shape[0], dim, _ptr(nbr), _ptr(order), rows, m, i0,
                                  KIND_CODES[kind], float(sigma2), phi_host, float(tau2), _ptr(values), _ptr(G),
                                  _ptr(partials), _ptr(grad), _ptr(workspace), workspace.numel(), _stream(dev)),
           "nngp_bf_grad_aniso")
    return partials, grad, G


def bf_grad_matern(coords: torch.Tensor, nbr: torch.Tensor, i0: int, sigma2: float, phi: float, tau2: float,
                   nu: float, values: torch.Tensor, want_rows: bool = False, order: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Gradient sweep of the general-smoothness Matern kind (``nngp_bf_grad_matern``, include/nngp.h) over rows
    ``i0 .. i0 + len(nbr)``, with the smoothness as a fourth parameter.

    Returns ``(partials, grad, G)``: the four partials of :func:`bf_sweep`, ``grad`` = the summed
    d loglik / d (sigma2, phi, tau2, nu) (float64 (4,), fixed fold order) and, with ``want_rows``, ``G`` (rows, 4)
    (NaN in rows flagged in partials[2]).  Stream-ordered on torch's current stream; no host synchronisation.
    0 < nu <= 50, 1 <= m <= 32; ``order`` as in :func:`bf_sweep`.  ``workspace`` (records and the three tables) may
    be reused across calls and across nu.
    """
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    if values is None or values.dtype != torch.float64 or values.shape != (coords.shape[0],):
        raise ValueError("values must be float64 (N,)")
    values = values.contiguous()
    rows, m = nbr.shape
    _check_kind("matern", nu)
    if not 1 <= m <= GRAD_MAX_M:
        raise NotImplementedError(f"the matern gradient sweep serves 1 <= m <= {GRAD_MAX_M} (m={m})")
    dev = _require_gpu(coords, nbr, values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    lib = load()
    need = lib.nngp_bf_grad_matern_workspace_bytes(rows, m)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    if workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous tensor on the sweep's device")
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    grad = torch.empty(4, dtype=torch.float64, device=dev)
    G = torch.empty((rows, 4), dtype=torch.float64, device=dev) if want_rows else None
    _check(lib.nngp_bf_grad_matern(_ptr(coords), coords.shape[0], coords.shape[1], _ptr(nbr), _ptr(order), rows, m, i0,
                                   float(sigma2), float(phi), float(tau2), float(nu), _ptr(values), _ptr(G),
                                   _ptr(partials), _ptr(grad), _ptr(workspace), workspace.numel(), _stream(dev)),
           "nngp_bf_grad_matern")
    return partials, grad, G


def matern_eval_d(u: torch.Tensor, nu: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(h, dnu)``: u rho'(u) and d rho / d nu of the Matern correlation, elementwise on the GPU through the
    gradient sweep's derivative table (``nngp_matern_eval_d``; u >= 0)."""
    if u.dtype != torch.float64:
        raise ValueError("u must be float64")
    dev = _require_gpu(u)
    _check_kind("matern", nu)
    u = u.contiguous()
    h = torch.empty_like(u)
    dnu = torch.empty_like(u)
    _check(load().nngp_matern_eval_d(_ptr(u), u.numel(), float(nu), _ptr(h), _ptr(dnu), _stream(dev)),
           "nngp_matern_eval_d")
    return h, dnu


def bf_dphi(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind: str, sigma2: float, phi: float, tau2: float,
            order: Optional[torch.Tensor] = None, B: Optional[torch.Tensor] = None, F: Optional[torch.Tensor] = None,
            dB: Optional[torch.Tensor] = None, dF: Optional[torch.Tensor] = None,
            workspace: Optional[torch.Tensor] = None):
    """The factors and their phi-derivatives in one sweep (``nngp_bf_dphi``, include/nngp.h) over rows ``i0 .. i0 +
    len(nbr)``: ``(B, F, dB, dF, partials)`` with dB = d B / d phi (rows, m), dF = d F / d phi (rows,) and partials
    = (sum log F, sum dF / F, first bad-pivot row or -1, first bad-index row or -1).  B and F equal
    :func:`bf_sweep`'s to that sweep's tolerance, not bit for bit.  ``B`` / ``F`` / ``dB`` / ``dF``: contiguous
    float64 outputs to write in place, or None.  Stream-ordered on torch's current stream; no host
    synchronisation.  Kinds exponential .. spherical, 1 <= m <= 32; ``order`` as in :func:`bf_sweep`."""
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    rows, m = nbr.shape
    if kind not in KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind == "matern":
        raise NotImplementedError("the phi-derivative sweep serves the kinds exponential .. spherical, not the "
                                  "general-nu matern kind")
    if not 1 <= m <= GRAD_MAX_M:
        raise NotImplementedError(f"the phi-derivative sweep serves 1 <= m <= {GRAD_MAX_M} (m={m})")
    dev = _require_gpu(coords, nbr, order, B, F, dB, dF)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    outs = []
    for t, shape, name in ((B, (rows, m), "B"), (F, (rows,), "F"), (dB, (rows, m), "dB"), (dF, (rows,), "dF")):
        if t is None:
            t = torch.empty(shape, dtype=torch.float64, device=dev)
        elif t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous float64 {shape}, got {t.dtype} {tuple(t.shape)}")
        outs.append(t)
    B, F, dB, dF = outs
    lib = load()
    need = lib.nngp_bf_dphi_workspace_bytes(rows, m)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    if workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous tensor on the sweep's device")
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    _check(lib.nngp_bf_dphi(_ptr(coords), coords.shape[0], coords.shape[1], _ptr(nbr), _ptr(order), rows, m, i0,
                            KIND_CODES[kind], float(sigma2), float(phi), float(tau2), _ptr(B), _ptr(F), _ptr(dB),
                            _ptr(dF), _ptr(partials), _ptr(workspace), workspace.numel(), _stream(dev)),
           "nngp_bf_dphi")
    return B, F, dB, dF, partials


def bf_fisher(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind: str, sigma2: float, phi: float, tau2: float,
              values: Optional[torch.Tensor] = None, want_rows: bool = False, order: Optional[torch.Tensor] = None,
              workspace: Optional[torch.Tensor] = None):
    """Fisher information sweep (``nngp_bf_fisher``, include/nngp.h) over rows ``i0 .. i0 + len(nbr)``.

    Returns ``(partials, grad, info, I_rows, G)``: the four partials of :func:`bf_grad`, ``grad`` (3,) = the summed
    d loglik / d (sigma2, phi, tau2), ``info`` (6,) = the summed expected information, upper triangle in the order
    (ss, sp, st, pp, pt, tt), and with ``want_rows`` the per-location terms ``I_rows`` (rows, 6) and ``G`` (rows, 3)
    at their natural rows (NaN in rows flagged in partials[2]), else None.  ``values=None`` gives the information
    alone: ``grad``, ``G`` and ``partials[1]`` are exactly 0.  Stream-ordered on torch's current stream; no host
    synchronisation.  Kinds exponential .. spherical, 1 <= m <= 32; ``order`` as in :func:`bf_sweep`.
    """
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    if values is not None:
        if values.dtype != torch.float64 or values.shape != (coords.shape[0],):
            raise ValueError("values must be float64 (N,) or None")
        values = values.contiguous()
    rows, m = nbr.shape
    if kind not in KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind == "matern":
        raise NotImplementedError("the information sweep serves the kinds exponential .. spherical, not the "
                                  "general-nu matern kind")
    if not 1 <= m <= GRAD_MAX_M:
        raise NotImplementedError(f"the information sweep serves 1 <= m <= {GRAD_MAX_M} (m={m})")
    dev = _require_gpu(coords, nbr, values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    lib = load()
    need = lib.nngp_bf_fisher_workspace_bytes(rows, m)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    if workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous tensor on the sweep's device")
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    grad = torch.empty(3, dtype=torch.float64, device=dev)
    info = torch.empty(6, dtype=torch.float64, device=dev)
    I_rows = torch.empty((rows, 6), dtype=torch.float64, device=dev) if want_rows else None
    G = torch.empty((rows, 3), dtype=torch.float64, device=dev) if want_rows else None
    _check(lib.nngp_bf_fisher(_ptr(coords), coords.shape[0], coords.shape[1], _ptr(nbr), _ptr(order), rows, m, i0,
                              KIND_CODES[kind], float(sigma2), float(phi), float(tau2), _ptr(values), _ptr(I_rows),
                              _ptr(G), _ptr(partials), _ptr(grad), _ptr(info), _ptr(workspace), workspace.numel(),
                              _stream(dev)),
           "nngp_bf_fisher")
    return partials, grad, info, I_rows, G


def nbr_cert(coords: torch.Tensor, nbr: torch.Tensor, i0: int = 0, order: Optional[torch.Tensor] = None):
    """A neighbour-set certificate (``nngp_nbr_cert_build``, include/nngp.h) for sweeps over exactly these
    (contiguous) tensors: ``(buffer, info)`` for :func:`bf_sweep`'s ``cert``.  A setup call (one host
    synchronisation).  The tensors must not be modified afterwards."""
    if not (coords.is_contiguous() and nbr.is_contiguous() and coords.dtype == torch.float64 and coords.dim() == 2
            and nbr.dtype == torch.int32 and nbr.dim() == 2):
        raise ValueError("nbr_cert needs contiguous float64 (N, dim) coords and int32 (rows, m) nbr")
    dev = _require_gpu(coords, nbr, order)
    rows, m = nbr.shape
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,) or not order.is_contiguous()):
        raise ValueError("order must be a contiguous int32 (rows,) tensor")
    lib = load()
    buf = _workspace(lib.nngp_nbr_cert_bytes(rows), dev)
    info = (ctypes.c_int64 * CERT_INFO_LEN)()
    _check(lib.nngp_nbr_cert_build(_ptr(coords), coords.shape[0], coords.shape[1], _ptr(nbr), _ptr(order), rows, m,
                                   int(i0), _ptr(buf), buf.numel(), info, _stream(dev)), "nngp_nbr_cert_build")
    return buf, info


def bf_finalize(workspace: torch.Tensor, rows: int, m: int, kind: str, dim: int, algo: str = "auto",
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fold the block records a ``bf_sweep(..., defer=True)`` left in ``workspace`` into
    ``out`` (float64 (4,)), on torch's current stream (nngp_bf_finalize).  ``rows``, ``m``,
    ``kind``, ``dim`` and ``algo`` must be the sweep's: they select the kernel, hence the record
    layout (the library checks the workspace size against them)."""
    dev = _require_gpu(workspace, out)
    out = torch.empty(4, dtype=torch.float64, device=dev) if out is None else out
    if not workspace.is_contiguous():
        raise ValueError("workspace must be contiguous")
    _check(load().nngp_bf_finalize(_ptr(workspace), workspace.numel() * workspace.element_size(), int(rows), int(m),
                                   KIND_CODES[kind], int(dim), ALGO_CODES[algo], _ptr(out), _stream(dev)),
           "nngp_bf_finalize")
    return out


def bf_cross(ref: torch.Tensor, query: torch.Tensor, nbr: torch.Tensor, kind: str, sigma2: float, phi: float,
             tau2: float = 0.0, ref_values: Optional[torch.Tensor] = None,
             query_values: Optional[torch.Tensor] = None, q0: int = 0, algo: str = "auto",
             B: Optional[torch.Tensor] = None, F: Optional[torch.Tensor] = None,
             partials: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
             order: Optional[torch.Tensor] = None,
             R: Optional[torch.Tensor] = None, nu: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """B_t, F_t of query rows ``q0 .. q0 + len(nbr)`` against the reference set ``ref``
    (nngp_bf_cross; prediction at t not in S).

    ``nbr[r]`` lists indices into ``ref`` (e.g. :func:`knn_query` output).  Returns
    ``(B, F, partials)``; with ``R`` given, ``R = query_values - B_t v_N`` (minus the
    kriging mean when ``query_values`` is None).
    """
    ref, query = _as_coords(ref), _as_coords(query)
    d = _same_dim(ref, query)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    if ref_values is not None:
        if ref_values.dtype != torch.float64 or ref_values.shape != (ref.shape[0],):
            raise ValueError("ref_values must be float64 (n_ref,)")
        ref_values = ref_values.contiguous()
    if query_values is not None:
        if query_values.dtype != torch.float64 or query_values.shape != (query.shape[0],):
            raise ValueError("query_values must be float64 (n_query,)")
        query_values = query_values.contiguous()
    dev = _require_gpu(ref, query, nbr, ref_values, query_values, order)
    rows, m = nbr.shape
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    nu = _check_kind(kind, nu)
    lib = load()
    a = ALGO_CODES[algo]
    _check_out(B, "B", (rows, m), dev)
    _check_out(F, "F", (rows,), dev)
    _check_out(partials, "partials", (4,), dev)
    _check_out(R, "R", (rows,), dev)
    B = torch.empty((rows, m), dtype=torch.float64, device=dev) if B is None else B
    F = torch.empty((rows,), dtype=torch.float64, device=dev) if F is None else F
    partials = torch.empty(4, dtype=torch.float64, device=dev) if partials is None else partials
    need = lib.nngp_bf_sweep_workspace_bytes(rows, m, KIND_CODES[kind], d, a)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    _check(lib.nngp_bf_cross(_ptr(ref), ref.shape[0], d, _ptr(query), query.shape[0], _ptr(nbr), _ptr(order), rows, m,
                             int(q0), KIND_CODES[kind], float(sigma2), float(phi), float(tau2), nu, _ptr(ref_values),
                             _ptr(query_values), _ptr(B), _ptr(F), _ptr(R), _ptr(partials), _ptr(workspace),
                             workspace.numel(), a, _stream(dev)), "nngp_bf_cross")
    return B, F, partials


def _noise_checks(kind: str, m: int) -> None:
    """The scope of the per-point noise sweeps (nngp_bf_*_noise): kinds exponential .. spherical, 1 <= m <= 32."""
    if kind not in KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind == "matern":
        raise NotImplementedError("the per-point noise sweeps serve the kinds exponential .. spherical, not the "
                                  "general-nu matern kind")
    if not 1 <= m <= GRAD_MAX_M:
        raise NotImplementedError(f"the per-point noise sweeps serve 1 <= m <= {GRAD_MAX_M} (m={m})")


def _noise_var(v: Optional[torch.Tensor], n: int, name: str) -> torch.Tensor:
    if v is None or v.dtype != torch.float64 or v.shape != (n,):
        raise ValueError(f"{name} must be float64 ({n},)")
    return v.contiguous()


def bf_sweep_noise(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind: str, sigma2: float, phi: float, tau2: float,
                   noise_var: torch.Tensor, values: Optional[torch.Tensor] = None, want_bf: bool = True,
                   order: Optional[torch.Tensor] = None, want_r: bool = False,
                   workspace: Optional[torch.Tensor] = None):
    """:func:`bf_sweep` with per-point noise (``nngp_bf_sweep_noise``, include/nngp.h): the noise variance of point j
    is ``tau2 * noise_var[j]`` (float64 (N,), >= 0), so every joint block's diagonal is ``sigma2 + tau2 v_j`` of the
    point in that slot.  Returns ``(B, F, R, partials)`` (B, F None without ``want_bf``; R None without ``want_r``,
    which needs ``values``).  Kinds exponential .. spherical, 1 <= m <= 32; ``order`` as in :func:`bf_sweep`.
    """
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    n = coords.shape[0]
    if values is not None:
        if values.dtype != torch.float64 or values.shape != (n,):
            raise ValueError("values must be float64 (N,)")
        values = values.contiguous()
    noise_var = _noise_var(noise_var, n, "noise_var")
    rows, m = nbr.shape
    _noise_checks(kind, m)
    dev = _require_gpu(coords, nbr, values, noise_var, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    if want_r and values is None:
        raise ValueError("want_r needs values")
    lib = load()
    need = lib.nngp_bf_sweep_noise_workspace_bytes(rows, m)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    B = torch.empty((rows, m), dtype=torch.float64, device=dev) if want_bf else None
    F = torch.empty((rows,), dtype=torch.float64, device=dev) if want_bf else None
    R = torch.empty((rows,), dtype=torch.float64, device=dev) if want_r else None
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    _check(lib.nngp_bf_sweep_noise(_ptr(coords), n, coords.shape[1], _ptr(nbr), _ptr(order), rows, m, int(i0),
                                   KIND_CODES[kind], float(sigma2), float(phi), float(tau2), _ptr(values),
                                   _ptr(noise_var), _ptr(B), _ptr(F), _ptr(R), _ptr(partials), _ptr(workspace),
                                   workspace.numel(), _stream(dev)), "nngp_bf_sweep_noise")
    return B, F, R, partials


def bf_grad_noise(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind: str, sigma2: float, phi: float, tau2: float,
                  values: torch.Tensor, noise_var: torch.Tensor, want_rows: bool = False,
                  order: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """:func:`bf_grad` with per-point noise (``nngp_bf_grad_noise``): ``(partials, grad, G)`` of the model whose
    noise variance at point j is ``tau2 * noise_var[j]``; grad in (sigma2, phi, tau2)."""
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    n = coords.shape[0]
    if values is None or values.dtype != torch.float64 or values.shape != (n,):
        raise ValueError("values must be float64 (N,)")
    values = values.contiguous()
    noise_var = _noise_var(noise_var, n, "noise_var")
    rows, m = nbr.shape
    _noise_checks(kind, m)
    dev = _require_gpu(coords, nbr, values, noise_var, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    lib = load()
    need = lib.nngp_bf_grad_workspace_bytes(rows, m)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    grad = torch.empty(3, dtype=torch.float64, device=dev)
    G = torch.empty((rows, 3), dtype=torch.float64, device=dev) if want_rows else None
    _check(lib.nngp_bf_grad_noise(_ptr(coords), n, coords.shape[1], _ptr(nbr), _ptr(order), rows, m, int(i0),
                                  KIND_CODES[kind], float(sigma2), float(phi), float(tau2), _ptr(values),
                                  _ptr(noise_var), _ptr(G), _ptr(partials), _ptr(grad), _ptr(workspace),
                                  workspace.numel(), _stream(dev)), "nngp_bf_grad_noise")
    return partials, grad, G


def bf_cross_noise(ref: torch.Tensor, query: torch.Tensor, nbr: torch.Tensor, kind: str, sigma2: float, phi: float,
                   tau2: float, noise_ref: torch.Tensor, noise_query: Optional[torch.Tensor] = None,
                   ref_values: Optional[torch.Tensor] = None, query_values: Optional[torch.Tensor] = None,
                   q0: int = 0, order: Optional[torch.Tensor] = None, want_r: bool = False):
    """:func:`bf_cross` with per-point noise (``nngp_bf_cross_noise``): ``noise_ref`` (n_ref,) weighs the neighbour
    block, ``noise_query`` (n_query,) or None (1) the query point's own diagonal entry.  Returns
    ``(B, F, R, partials)`` (R None without ``want_r``, which needs ``ref_values``)."""
    ref, query = _as_coords(ref), _as_coords(query)
    d = _same_dim(ref, query)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    if ref_values is not None:
        if ref_values.dtype != torch.float64 or ref_values.shape != (ref.shape[0],):
            raise ValueError("ref_values must be float64 (n_ref,)")
        ref_values = ref_values.contiguous()
    if query_values is not None:
        if query_values.dtype != torch.float64 or query_values.shape != (query.shape[0],):
            raise ValueError("query_values must be float64 (n_query,)")
        query_values = query_values.contiguous()
    noise_ref = _noise_var(noise_ref, ref.shape[0], "noise_ref")
    if noise_query is not None:
        noise_query = _noise_var(noise_query, query.shape[0], "noise_query")
    rows, m = nbr.shape
    _noise_checks(kind, m)
    dev = _require_gpu(ref, query, nbr, ref_values, query_values, noise_ref, noise_query, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    if want_r and ref_values is None:
        raise ValueError("want_r needs ref_values")
    lib = load()
    B = torch.empty((rows, m), dtype=torch.float64, device=dev)
    F = torch.empty((rows,), dtype=torch.float64, device=dev)
    R = torch.empty((rows,), dtype=torch.float64, device=dev) if want_r else None
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    workspace = _workspace(lib.nngp_bf_sweep_noise_workspace_bytes(rows, m), dev)
    _check(lib.nngp_bf_cross_noise(_ptr(ref), ref.shape[0], d, _ptr(query), query.shape[0], _ptr(nbr), _ptr(order), rows,
                                   m, int(q0), KIND_CODES[kind], float(sigma2), float(phi), float(tau2),
                                   _ptr(ref_values), _ptr(query_values), _ptr(noise_ref), _ptr(noise_query), _ptr(B),
                                   _ptr(F), _ptr(R), _ptr(partials), _ptr(workspace), workspace.numel(), _stream(dev)),
           "nngp_bf_cross_noise")
    return B, F, R, partials


def _sep_checks(kind_s: str, kind_t: str, m: int, dim: int) -> None:
    """The scope of the separable space-time sweeps (nngp_bf_*_sep): factors exponential .. spherical, dim 2 or 3,
    1 <= m <= 32."""
    for k in (kind_s, kind_t):
        if k not in KIND_CODES:
            raise ValueError(f"unknown covariance kind {k!r}")
        if k == "matern":
            raise NotImplementedError("the separable sweeps serve factors of kind exponential .. spherical, not the "
                                      "general-nu matern kind")
    if dim not in (2, 3):
        raise NotImplementedError(f"the separable sweeps serve dim 2 or 3 (space, then time in the last column), "
                                  f"dim={dim}")
    if not 1 <= m <= GRAD_MAX_M:
        raise NotImplementedError(f"the separable sweeps serve 1 <= m <= {GRAD_MAX_M} (m={m})")


def bf_sweep_sep(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind_s: str, kind_t: str, sigma2: float,
                 phi_s: float, phi_t: float, tau2: float, values: Optional[torch.Tensor] = None, want_bf: bool = True,
                 order: Optional[torch.Tensor] = None, want_r: bool = False,
                 workspace: Optional[torch.Tensor] = None):
    """:func:`bf_sweep` under the separable space-time covariance (``nngp_bf_sweep_sep``, include/nngp.h):
    ``sigma2 rho_s(phi_s |a_s - b_s|) rho_t(phi_t |a_t - b_t|) + tau2 delta_ab`` with the time in the last column of
    ``coords`` (dim 2 or 3).  Returns ``(B, F, R, partials)`` (B, F None without ``want_bf``; R None without
    ``want_r``, which needs ``values``).  Factors exponential .. spherical, 1 <= m <= 32; ``order`` as in
    :func:`bf_sweep`."""
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    n = coords.shape[0]
    if values is not None:
        if values.dtype != torch.float64 or values.shape != (n,):
            raise ValueError("values must be float64 (N,)")
        values = values.contiguous()
    rows, m = nbr.shape
    _sep_checks(kind_s, kind_t, m, coords.shape[1])
    dev = _require_gpu(coords, nbr, values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    if want_r and values is None:
        raise ValueError("want_r needs values")
    lib = load()
    need = lib.nngp_bf_sweep_sep_workspace_bytes(rows, m)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    B = torch.empty((rows, m), dtype=torch.float64, device=dev) if want_bf else None
    F = torch.empty((rows,), dtype=torch.float64, device=dev) if want_bf else None
    R = torch.empty((rows,), dtype=torch.float64, device=dev) if want_r else None
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    _check(lib.nngp_bf_sweep_sep(_ptr(coords), n, coords.shape[1], _ptr(nbr), _ptr(order), rows, m, int(i0),
                                 KIND_CODES[kind_s], KIND_CODES[kind_t], float(sigma2), float(phi_s), float(phi_t),
                                 float(tau2), _ptr(values), _ptr(B), _ptr(F), _ptr(R), _ptr(partials), _ptr(workspace),
                                 workspace.numel(), _stream(dev)), "nngp_bf_sweep_sep")
    return B, F, R, partials


def bf_grad_sep(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind_s: str, kind_t: str, sigma2: float,
                phi_s: float, phi_t: float, tau2: float, values: torch.Tensor, want_rows: bool = False,
                order: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """:func:`bf_grad` under the separable space-time covariance (``nngp_bf_grad_sep``): ``(partials, grad, G)`` with
    grad (4,) and G (rows, 4) in (sigma2, phi_s, phi_t, tau2)."""
    coords = _as_coords(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    n = coords.shape[0]
    if values is None or values.dtype != torch.float64 or values.shape != (n,):
        raise ValueError("values must be float64 (N,)")
    values = values.contiguous()
    rows, m = nbr.shape
    _sep_checks(kind_s, kind_t, m, coords.shape[1])
    dev = _require_gpu(coords, nbr, values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    lib = load()
    need = lib.nngp_bf_sweep_sep_workspace_bytes(rows, m)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    grad = torch.empty(4, dtype=torch.float64, device=dev)
    G = torch.empty((rows, 4), dtype=torch.float64, device=dev) if want_rows else None
    _check(lib.nngp_bf_grad_sep(_ptr(coords), n, coords.shape[1], _ptr(nbr), _ptr(order), rows, m, int(i0),
                                KIND_CODES[kind_s], KIND_CODES[kind_t], float(sigma2), float(phi_s), float(phi_t),
                                float(tau2), _ptr(values), _ptr(G), _ptr(partials), _ptr(grad), _ptr(workspace),
                                workspace.numel(), _stream(dev)), "nngp_bf_grad_sep")
    return partials, grad, G


def bf_cross_sep(ref: torch.Tensor, query: torch.Tensor, nbr: torch.Tensor, kind_s: str, kind_t: str, sigma2: float,
                 phi_s: float, phi_t: float, tau2: float, ref_values: Optional[torch.Tensor] = None,
                 query_values: Optional[torch.Tensor] = None, q0: int = 0, order: Optional[torch.Tensor] = None,
                 want_r: bool = False):
    """:func:`bf_cross` under the separable space-time covariance (``nngp_bf_cross_sep``).  Returns
    ``(B, F, R, partials)`` (R None without ``want_r``, which needs ``ref_values``)."""
    ref, query = _as_coords(ref), _as_coords(query)
    d = _same_dim(ref, query)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    if ref_values is not None:
        if ref_values.dtype != torch.float64 or ref_values.shape != (ref.shape[0],):
            raise ValueError("ref_values must be float64 (n_ref,)")
        ref_values = ref_values.contiguous()
    if query_values is not None:
        if query_values.dtype != torch.float64 or query_values.shape != (query.shape[0],):
            raise ValueError("query_values must be float64 (n_query,)")
        query_values = query_values.contiguous()
    rows, m = nbr.shape
    _sep_checks(kind_s, kind_t, m, d)
    dev = _require_gpu(ref, query, nbr, ref_values, query_values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    if want_r and ref_values is None:
        raise ValueError("want_r needs ref_values")
    lib = load()
    B = torch.empty((rows, m), dtype=torch.float64, device=dev)
    F = torch.empty((rows,), dtype=torch.float64, device=dev)
    R = torch.empty((rows,), dtype=torch.float64, device=dev) if want_r else None
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    workspace = _workspace(lib.nngp_bf_sweep_sep_workspace_bytes(rows, m), dev)
    _check(lib.nngp_bf_cross_sep(_ptr(ref), ref.shape[0], d, _ptr(query), query.shape[0], _ptr(nbr), _ptr(order), rows, m,
                                 int(q0), KIND_CODES[kind_s], KIND_CODES[kind_t], float(sigma2), float(phi_s),
                                 float(phi_t), float(tau2), _ptr(ref_values), _ptr(query_values), _ptr(B), _ptr(F),
                                 _ptr(R), _ptr(partials), _ptr(workspace), workspace.numel(), _stream(dev)),
           "nngp_bf_cross_sep")
    return B, F, R, partials


# ---------------------------------------------------------------- points in 4 .. 16 dimensions (nngp_*_nd)
def _as_coords_nd(coords: torch.Tensor) -> torch.Tensor:
    """float64 (N, dim) ordinates, ND_MIN_DIM <= dim <= ND_MAX_DIM."""
    if coords.dim() != 2 or not ND_MIN_DIM <= coords.shape[1] <= ND_MAX_DIM or coords.dtype != torch.float64:
        raise ValueError(f"coords must be float64 (N, dim), {ND_MIN_DIM} <= dim <= {ND_MAX_DIM}, got "
                         f"{tuple(coords.shape)} {coords.dtype}")
    return coords.contiguous()


def _nd_checks(kind: str, m: int, dim: int, phi) -> "ctypes.Array":
    """The scope of the n-dimensional sweeps (nngp_bf_*_nd); returns the decays as a C array."""
    if kind not in KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind == "spherical":
        raise NotImplementedError("the spherical correlation is not positive definite above three dimensions: the "
                                  "n-dimensional sweeps refuse it")
    if kind not in ND_KINDS:
        raise NotImplementedError(f"the n-dimensional sweeps serve the kinds {ND_KINDS}, not {kind!r}")
    if not 1 <= m <= GRAD_MAX_M:
        raise NotImplementedError(f"the n-dimensional sweeps serve 1 <= m <= {GRAD_MAX_M} (m={m})")
    phi = [float(x) for x in phi]
    if len(phi) != dim:
        raise ValueError(f"phi must hold one decay per coordinate column ({dim}), got {len(phi)}")
    return (ctypes.c_double * dim)(*phi)


def knn_prior_nd(coords: torch.Tensor, m: int, q0: int = 0, q1: Optional[int] = None) -> torch.Tensor:
    """:func:`knn_prior` for 4 .. 16 coordinate columns (``nngp_knn_prior_nd``: exact, tiled brute force)."""
    coords = _as_coords_nd(coords)
    dev = _require_gpu(coords)
    n, d = coords.shape
    q1 = n if q1 is None else int(q1)
    if not 0 <= q0 <= q1 <= n:
        raise ValueError(f"query rows [{q0}, {q1}) outside [0, {n})")
    out = torch.empty((q1 - q0, m), dtype=torch.int32, device=dev)
    lib = load()
    ws = _workspace(lib.nngp_knn_nd_workspace_bytes(n, d, m), dev)
    _check(lib.nngp_knn_prior_nd(_ptr(coords), n, d, m, q0, q1, _ptr(out), _ptr(ws), ws.numel(), _stream(dev)),
           "nngp_knn_prior_nd")
    return out


def knn_query_nd(ref: torch.Tensor, query: torch.Tensor, k: int) -> torch.Tensor:
    """:func:`knn_query` for 4 .. 16 coordinate columns (``nngp_knn_query_nd``)."""
    ref, query = _as_coords_nd(ref), _as_coords_nd(query)
    d = _same_dim(ref, query)
    dev = _require_gpu(ref, query)
    out = torch.empty((query.shape[0], k), dtype=torch.int32, device=dev)
    lib = load()
    ws = _workspace(lib.nngp_knn_nd_workspace_bytes(ref.shape[0], d, k), dev)
    _check(lib.nngp_knn_query_nd(_ptr(ref), ref.shape[0], d, _ptr(query), query.shape[0], k, _ptr(out), _ptr(ws),
                                 ws.numel(), _stream(dev)), "nngp_knn_query_nd")
    return out


def bf_sweep_nd(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind: str, sigma2: float, phi, tau2: float,
                values: Optional[torch.Tensor] = None, want_bf: bool = True, order: Optional[torch.Tensor] = None,
                want_r: bool = False, workspace: Optional[torch.Tensor] = None):
    """:func:`bf_sweep` for 4 .. 16 coordinate columns with one decay per column (``nngp_bf_sweep_nd``,
    include/nngp.h): ``sigma2 rho(sqrt(sum_k (phi_k d_k)^2)) + tau2 delta_ab``.  ``phi`` is a sequence of ``dim``
    floats.  Returns ``(B, F, R, partials)`` (B, F None without ``want_bf``; R None without ``want_r``, which needs
    ``values``).  Kinds exponential, matern32, matern52, gaussian; 1 <= m <= 32; ``order`` as in :func:`bf_sweep`."""
    coords = _as_coords_nd(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    n, d = coords.shape
    if values is not None:
        if values.dtype != torch.float64 or values.shape != (n,):
            raise ValueError("values must be float64 (N,)")
        values = values.contiguous()
    rows, m = nbr.shape
    cphi = _nd_checks(kind, m, d, phi)
    dev = _require_gpu(coords, nbr, values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    if want_r and values is None:
        raise ValueError("want_r needs values")
    lib = load()
    need = lib.nngp_bf_sweep_nd_workspace_bytes(rows, m, d)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    B = torch.empty((rows, m), dtype=torch.float64, device=dev) if want_bf else None
    F = torch.empty((rows,), dtype=torch.float64, device=dev) if want_bf else None
    R = torch.empty((rows,), dtype=torch.float64, device=dev) if want_r else None
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    _check(lib.nngp_bf_sweep_nd(_ptr(coords), n, d, _ptr(nbr), _ptr(order), rows, m, int(i0), KIND_CODES[kind],
                                float(sigma2), cphi, float(tau2), _ptr(values), _ptr(B), _ptr(F), _ptr(R),
                                _ptr(partials), _ptr(workspace), workspace.numel(), _stream(dev)), "nngp_bf_sweep_nd")
    return B, F, R, partials


def bf_grad_nd(coords: torch.Tensor, nbr: torch.Tensor, i0: int, kind: str, sigma2: float, phi, tau2: float,
               values: torch.Tensor, want_rows: bool = False, order: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """:func:`bf_grad_aniso` for 4 .. 16 coordinate columns (``nngp_bf_grad_nd``): ``(partials, grad, G)`` with grad
    (dim + 2,) and G (rows, dim + 2) in (sigma2, phi_1..phi_dim, tau2)."""
    coords = _as_coords_nd(coords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    n, d = coords.shape
    if values is None or values.dtype != torch.float64 or values.shape != (n,):
        raise ValueError("values must be float64 (N,)")
    values = values.contiguous()
    rows, m = nbr.shape
    cphi = _nd_checks(kind, m, d, phi)
    dev = _require_gpu(coords, nbr, values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    lib = load()
    need = lib.nngp_bf_sweep_nd_workspace_bytes(rows, m, d)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    grad = torch.empty(d + 2, dtype=torch.float64, device=dev)
    G = torch.empty((rows, d + 2), dtype=torch.float64, device=dev) if want_rows else None
    _check(lib.nngp_bf_grad_nd(_ptr(coords), n, d, _ptr(nbr), _ptr(order), rows, m, int(i0), KIND_CODES[kind],
                               float(sigma2), cphi, float(tau2), _ptr(values), _ptr(G), _ptr(partials), _ptr(grad),
                               _ptr(workspace), workspace.numel(), _stream(dev)), "nngp_bf_grad_nd")
    return partials, grad, G


def bf_cross_nd(ref: torch.Tensor, query: torch.Tensor, nbr: torch.Tensor, kind: str, sigma2: float, phi, tau2: float,
                ref_values: Optional[torch.Tensor] = None, query_values: Optional[torch.Tensor] = None, q0: int = 0,
                order: Optional[torch.Tensor] = None, want_r: bool = False):
    """:func:`bf_cross` for 4 .. 16 coordinate columns (``nngp_bf_cross_nd``).  Returns ``(B, F, R, partials)`` (R None
    without ``want_r``, which needs ``ref_values``)."""
    ref, query = _as_coords_nd(ref), _as_coords_nd(query)
    d = _same_dim(ref, query)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    if ref_values is not None:
        if ref_values.dtype != torch.float64 or ref_values.shape != (ref.shape[0],):
            raise ValueError("ref_values must be float64 (n_ref,)")
        ref_values = ref_values.contiguous()
    if query_values is not None:
        if query_values.dtype != torch.float64 or query_values.shape != (query.shape[0],):
            raise ValueError("query_values must be float64 (n_query,)")
        query_values = query_values.contiguous()
    rows, m = nbr.shape
    cphi = _nd_checks(kind, m, d, phi)
    dev = _require_gpu(ref, query, nbr, ref_values, query_values, order)
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    if want_r and ref_values is None:
        raise ValueError("want_r needs ref_values")
    lib = load()
    B = torch.empty((rows, m), dtype=torch.float64, device=dev)
    F = torch.empty((rows,), dtype=torch.float64, device=dev)
    R = torch.empty((rows,), dtype=torch.float64, device=dev) if want_r else None
    partials = torch.empty(4, dtype=torch.float64, device=dev)
    workspace = _workspace(lib.nngp_bf_sweep_nd_workspace_bytes(rows, m, d), dev)
    _check(lib.nngp_bf_cross_nd(_ptr(ref), ref.shape[0], d, _ptr(query), query.shape[0], _ptr(nbr), _ptr(order), rows, m,
                                int(q0), KIND_CODES[kind], float(sigma2), cphi, float(tau2), _ptr(ref_values),
                                _ptr(query_values), _ptr(B), _ptr(F), _ptr(R), _ptr(partials), _ptr(workspace),
                                workspace.numel(), _stream(dev)), "nngp_bf_cross_nd")
    return B, F, R, partials


def joint_dist(coords: torch.Tensor, nbr: torch.Tensor, i0: int = 0, qcoords: Optional[torch.Tensor] = None,
               order: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Distances of every joint block (nngp_joint_dist): float64 ((m+1)(m+2)/2, rows), entry
    (a, b), b <= a, of nbr row t at ``[a (a+1)/2 + b, t]`` (row m of a block is the location
    ``i0 + (order[t] if order else t)``, taken from ``qcoords``, default ``coords``); 0 on the
    diagonal, +inf for slots without a point.  Map it through a covariance function and pass
    the result to :func:`bf_sweep_blocks`."""
    coords = _as_coords(coords)
    qcoords = coords if qcoords is None else _as_coords(qcoords)
    d = _same_dim(coords, qcoords)
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    dev = _require_gpu(coords, qcoords, nbr, order)
    rows, m = nbr.shape
    if order is not None and (order.dtype != torch.int32 or order.shape != (rows,)):
        raise ValueError("order must be int32 (rows,)")
    lib = load()
    ne = int(lib.nngp_joint_entries(m))
    _check_out(out, "out", (ne, rows), dev)
    out = torch.empty((ne, rows), dtype=torch.float64, device=dev) if out is None else out
    _check(lib.nngp_joint_dist(_ptr(coords), coords.shape[0], d, _ptr(qcoords), qcoords.shape[0], _ptr(nbr),
                               _ptr(order), rows, m, int(i0), _ptr(out), _stream(dev)), "nngp_joint_dist")
    return out


def matern(u: torch.Tensor, nu: float) -> torch.Tensor:
    """u^nu K_nu(u) / (2^(nu-1) Gamma(nu)) elementwise on the GPU (nngp_matern_eval; u >= 0, +inf -> 0),
    e.g. ``IsotropicCovariance(lambda d: s2 * matern(phi * d, nu), tau2)``."""
    if u.dtype != torch.float64:
        raise ValueError("u must be float64")
    dev = _require_gpu(u)
    _check_kind("matern", nu)
    u = u.contiguous()
    out = torch.empty_like(u)
    _check(load().nngp_matern_eval(_ptr(u), u.numel(), float(nu), _ptr(out), _stream(dev)), "nngp_matern_eval")
    return out


def joint_diagonal(m: int) -> torch.Tensor:
    """Row indices a (a+1)/2 + a of the diagonal entries of a joint block (for adding a nugget)."""
    a = torch.arange(m + 1)
    return a * (a + 1) // 2 + a


def bf_sweep_blocks(cov: torch.Tensor, nbr: torch.Tensor, n_points: int, i0: int = 0,
                    values: Optional[torch.Tensor] = None, qvalues: Optional[torch.Tensor] = None,
                    want_bf: bool = True, order: Optional[torch.Tensor] = None, R: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None, n_locs: Optional[int] = None,
                    B: Optional[torch.Tensor] = None, F: Optional[torch.Tensor] = None,
                    partials: Optional[torch.Tensor] = None
                    ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], torch.Tensor]:
    """The fused B/F + log-lik sweep with the joint blocks' covariances given (nngp_bf_sweep_blocks):
    ``cov`` float64 ((m+1)(m+2)/2, rows) in :func:`joint_dist`'s layout (the covariance function
    of the distances, the nugget on the diagonal entries).  ``values`` (n_points,) at the
    neighbours and ``qvalues`` (n_locs,) at the locations (pass ``values`` again for the S = T
    sweep; None: 0, so R = -B v_N, minus the kriging mean).
    Returns ``(B, F, partials)`` as :func:`bf_sweep`.  1 <= m <= 32 (the two-lane kernel up to 24,
    the four-lane kernel above).  The C ABI takes raw pointers, so every length is checked here:
    ``values`` (n_points,), ``qvalues`` (n_locs,), ``order`` int32 (rows,)."""
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError(f"nbr must be int32 (rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    nbr = nbr.contiguous()
    rows, m = nbr.shape
    lib = load()
    ne = int(lib.nngp_joint_entries(m))
    if cov.dtype != torch.float64 or tuple(cov.shape) != (ne, rows):
        raise ValueError(f"cov must be float64 ({ne}, {rows}) (joint_dist's layout), got {cov.dtype} {tuple(cov.shape)}")
    cov = cov.contiguous()
    n_locs = int(n_points if n_locs is None else n_locs)
    for name, v, n in (("values", values, n_points), ("qvalues", qvalues, n_locs)):
        if v is not None and (v.dtype != torch.float64 or tuple(v.shape) != (int(n),)):
            raise ValueError(f"{name} must be float64 of shape ({int(n)},), got {v.dtype} {tuple(v.shape)}")
    if order is not None:
        if order.dtype != torch.int32 or tuple(order.shape) != (rows,):
            raise ValueError(f"order must be int32 of shape ({rows},), got {order.dtype} {tuple(order.shape)}")
        order = order.contiguous()
    values = None if values is None else values.contiguous()
    qvalues = None if qvalues is None else qvalues.contiguous()
    dev = _require_gpu(cov, nbr, values, qvalues, order, R)
    if want_bf:
        _check_out(B, "B", (rows, m), dev)
        _check_out(F, "F", (rows,), dev)
        B = torch.empty((rows, m), dtype=torch.float64, device=dev) if B is None else B
        F = torch.empty((rows,), dtype=torch.float64, device=dev) if F is None else F
    else:
        B = F = None
    _check_out(R, "R", (rows,), dev)
    _check_out(partials, "partials", (4,), dev)
    partials = torch.empty(4, dtype=torch.float64, device=dev) if partials is None else partials
    need = lib.nngp_bf_sweep_blocks_workspace_bytes(rows)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    _check(lib.nngp_bf_sweep_blocks(_ptr(cov), _ptr(nbr), _ptr(order), int(n_points), rows, m, int(i0), n_locs,
                                    _ptr(values), _ptr(qvalues), _ptr(B), _ptr(F), _ptr(R), _ptr(partials),
                                    _ptr(workspace), workspace.numel(), _stream(dev)), "nngp_bf_sweep_blocks")
    return B, F, partials


def row_order(coords: torch.Tensor, i0: int = 0, rows: Optional[int] = None,
              nbr: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Z-order visiting order of locations i0 .. i0+rows-1 for :func:`bf_sweep`.

    Returns ``(order, nbr_sorted)``: ``order`` int32 (rows,) and, when ``nbr`` (the
    natural-order neighbour rows of those locations) is given, ``nbr_sorted[t] =
    nbr[order[t]]``.  Sweep with ``bf_sweep(coords, nbr_sorted, i0, ..., order=order)``.
    """
    coords = _as_coords(coords)
    dev = _require_gpu(coords, nbr)
    n = coords.shape[0]
    rows = n - i0 if rows is None else int(rows)
    m = 0 if nbr is None else nbr.shape[1]
    if nbr is not None:
        if nbr.dtype != torch.int32 or nbr.shape[0] != rows:
            raise ValueError("nbr must be int32 (rows, m)")
        nbr = nbr.contiguous()
    out = torch.empty((rows,), dtype=torch.int32, device=dev)
    srt = None if nbr is None else torch.empty_like(nbr)
    lib = load()
    need = lib.nngp_row_order_workspace_bytes(rows)
    if need == 0:
        raise NNGPExtensionError("nngp_row_order_workspace_bytes failed")
    ws = _workspace(need, dev)
    _check(lib.nngp_row_order(_ptr(coords), n, coords.shape[1], _ptr(nbr), m, i0, rows, _ptr(out), _ptr(srt), _ptr(ws),
                              ws.numel(), _stream(dev)), "nngp_row_order")
    return out, srt


MAXMIN_TAIL = 20  # level of the points no level of the max-min order selected
MAXMIN_STATS_LEN = 64  # int32 counters nngp_order_maxmin leaves at the head of its workspace


def order_maxmin(coords: torch.Tensor, seed: int = 0, want_stats: bool = False):
    """Levelled max-min order of ``coords`` (``nngp_order_maxmin``, include/nngp.h):
    ``(perm, level)``, ``perm`` int64 (n,) with ``perm[k]`` the input row at position k and ``level`` int32 (n,) the
    level of the point at position k (0 for the first point, 1 .. 19, 20 for the tail).  A setup call: it
    synchronises the current stream once per round.  ``want_stats``: also a dict of what the call did (launches,
    count reads, rounds / accept-retire iterations / points selected per level)."""
    coords = _as_coords(coords)
    dev = _require_gpu(coords)
    n, d = coords.shape
    if n < 1:
        raise ValueError("order_maxmin needs at least one point")
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError(f"seed must be a uint32, got {seed}")
    lib = load()
    need = lib.nngp_order_maxmin_workspace_bytes(n, d)
    if need == 0:
        raise NNGPExtensionError("nngp_order_maxmin_workspace_bytes failed")
    ws = _workspace(need, dev)
    perm = torch.empty((n,), dtype=torch.int64, device=dev)
    level = torch.empty((n,), dtype=torch.int32, device=dev)
    _check(lib.nngp_order_maxmin(_ptr(coords), n, d, int(seed), _ptr(perm), _ptr(level), _ptr(ws), ws.numel(),
                                 _stream(dev)), "nngp_order_maxmin")
    if not want_stats:
        return perm, level
    st = ws[:4 * MAXMIN_STATS_LEN].view(torch.int32).cpu().tolist()
    stats = {"launches": st[0], "host_reads": st[1], "levels": st[2], "n_tail": st[3], "rounds": st[4:24],
             "accept_iterations": st[24:44], "selected": st[44:64]}
    return perm, level, stats


def combine_partials(gathered: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rank-order fold of all-gathered (world, 4) partials into (4,) (one tiny kernel)."""
    if gathered.dtype != torch.float64 or gathered.dim() != 2 or gathered.shape[1] != 4:
        raise ValueError("gathered must be float64 (world, 4)")
    gathered = gathered.contiguous()
    dev = _require_gpu(gathered, out)
    out = torch.empty(4, dtype=torch.float64, device=dev) if out is None else out
    _check(load().nngp_combine_partials(_ptr(gathered), gathered.shape[0], _ptr(out), _stream(dev)),
           "nngp_combine_partials")
    return out


def bf_workspace(rows: int, m: int, algo: str, device, kind: Optional[str] = None, dim: int = 2) -> torch.Tensor:
    """Pre-allocate a sweep workspace (reuse it across calls in a hot loop); ``kind=None``
    sizes it for any covariance kind."""
    kinds = KIND_CODES.values() if kind is None else (KIND_CODES[kind],)
    need = max(load().nngp_bf_sweep_workspace_bytes(rows, m, k, int(dim), ALGO_CODES[algo]) for k in kinds)
    return _workspace(need, torch.device(device))


# ---------------------------------------------------------------------------- Gibbs sampler pieces
def reverse_neighbors(nbr: torch.Tensor):
    """CSR transpose of the neighbour sets: (off (n+1,), rev_j (n*m,), rev_k (n*m,)) int32 on the device."""
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError("nbr must be int32 (n, m)")
    nbr = nbr.contiguous()
    dev = _require_gpu(nbr)
    n, m = nbr.shape
    off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    rev_j = torch.empty(max(n * m, 1), dtype=torch.int32, device=dev)
    rev_k = torch.empty(max(n * m, 1), dtype=torch.int32, device=dev)
    lib = load()
    need = lib.nngp_reverse_workspace_bytes(n, m)
    if need == 0:
        raise NNGPExtensionError("nngp_reverse_workspace_bytes failed")
    ws = _workspace(need, dev)
    _check(lib.nngp_reverse_neighbors(_ptr(nbr), n, m, _ptr(off), _ptr(rev_j), _ptr(rev_k), _ptr(ws), ws.numel(),
                                      _stream(dev)), "nngp_reverse_neighbors")
    return off, rev_j, rev_k


def color_moral_graph(nbr_host, off_host, rev_j_host):
    """Greedy moral-graph colouring on the host (numpy int32 inputs); returns (colors, n_colors)."""
    import numpy as np

    nbr_host = np.ascontiguousarray(nbr_host, dtype=np.int32)
    off_host = np.ascontiguousarray(off_host, dtype=np.int32)
    rev_j_host = np.ascontiguousarray(rev_j_host, dtype=np.int32)
    n, m = nbr_host.shape
    colors = np.empty(n, dtype=np.int32)
    nc = load().nngp_color_moral_graph(nbr_host.ctypes.data, off_host.ctypes.data, rev_j_host.ctypes.data, n, m,
                                       colors.ctypes.data)
    if nc < 0:
        _check(int(nc), "nngp_color_moral_graph")
    return colors, int(nc)


def color_moral_graph_dev(nbr: torch.Tensor, off: torch.Tensor, rev_j: torch.Tensor):
    """:func:`color_moral_graph` on the device (nngp_color_moral_graph_dev, the same colours bit for bit):
    (colors int32 (n,) device tensor, n_colors).  Falls back to the host greedy past 256 colours."""
    if nbr.dtype != torch.int32 or nbr.dim() != 2:
        raise ValueError("nbr must be int32 (n, m)")
    dev = _require_gpu(nbr, off, rev_j)
    n, m = nbr.shape
    color = torch.empty(n, dtype=torch.int32, device=dev)
    ws = _workspace(256, dev)
    nc = load().nngp_color_moral_graph_dev(_ptr(nbr.contiguous()), _ptr(off), _ptr(rev_j), n, m, _ptr(color), _ptr(ws),
                                           ws.numel(), _stream(dev))
    if nc == -4:  # NNGP_EUNSUP: more than 256 colours
        c, k = color_moral_graph(nbr.cpu().numpy(), off.cpu().numpy(), rev_j.cpu().numpy())
        return torch.from_numpy(c).to(dev), k
    _check(0 if nc >= 0 else int(nc), "nngp_color_moral_graph_dev")
    return color, int(nc)


def gibbs_prepare(B: torch.Tensor, Ft: torch.Tensor, off: torch.Tensor, rev_j: torch.Tensor, rev_k: torch.Tensor,
                  prep: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fold the unit-variance factors (B, Ft) into the reverse-list layout the w sweeps read
    (nngp_gibbs_prepare); returns the device buffer to pass to :func:`gibbs_w_sweep`."""
    dev = _require_gpu(B, Ft, off, rev_j, rev_k, prep, order)
    n, m = B.shape
    if order is not None and (order.dtype != torch.int32 or order.shape != (n,)):
        raise ValueError("order must be int32 (n,)")
    lib = load()
    need = lib.nngp_gibbs_prep_bytes(n, m)
    if prep is None or prep.numel() < need:
        prep = _workspace(need, dev)
    _check(lib.nngp_gibbs_prepare(_ptr(B), _ptr(Ft), _ptr(off), _ptr(rev_j), _ptr(rev_k), _ptr(order), n, m, _ptr(prep),
                                  prep.numel(), _stream(dev)), "nngp_gibbs_prepare")
    return prep


def gibbs_prepare_range(B: torch.Tensor, Ft: torch.Tensor, off: torch.Tensor, rev_j: torch.Tensor,
                        rev_k: torch.Tensor, row0: int, row1: int, prep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`gibbs_prepare` for the rows [row0, row1) only (nngp_gibbs_prepare_range): a rank's
    own shard of a sharded chain.  ``prep`` keeps the whole-field layout."""
    dev = _require_gpu(B, Ft, off, rev_j, rev_k, prep)
    n, m = B.shape
    lib = load()
    need = lib.nngp_gibbs_prep_bytes(n, m)
    if prep is None or prep.numel() < need:
        prep = _workspace(need, dev)
    _check(lib.nngp_gibbs_prepare_range(_ptr(B), _ptr(Ft), _ptr(off), _ptr(rev_j), _ptr(rev_k), n, m, int(row0),
                                        int(row1), _ptr(prep), prep.numel(), _stream(dev)), "nngp_gibbs_prepare_range")
    return prep


def gibbs_w_color(member_rows: torch.Tensor, prep: torch.Tensor, m: int, sigma2: float, tau2: float,
                  yres: torch.Tensor, w: torch.Tensor, r: torch.Tensor, rev_j: torch.Tensor, seed: int, sweep: int,
                  z: Optional[torch.Tensor] = None, noise_w: Optional[torch.Tensor] = None,
                  w_out: Optional[torch.Tensor] = None) -> None:
    """ONE colour step over ``member_rows`` (rows of :func:`gibbs_member_rows`), in place on w, r;
    ``w_out`` (len(member_rows),) receives the members' new w (nngp_gibbs_w_color)."""
    dev = _require_gpu(member_rows, prep, yres, w, r, rev_j, z, noise_w, w_out)
    _check_noise_w(noise_w, w.shape[0])
    k = member_rows.shape[0]
    if member_rows.dtype != torch.int32 or member_rows.dim() != 2 or member_rows.shape[1] != 4 \
            or not member_rows.is_contiguous():
        raise ValueError("member_rows must be a contiguous int32 (k, 4) tensor")
    _check_out(w_out, "w_out", (k,), dev)
    _check(load().nngp_gibbs_w_color(_ptr(member_rows), k, _ptr(prep), w.shape[0], int(m), float(sigma2), float(tau2),
                                     _ptr(yres), _ptr(noise_w), _ptr(w), _ptr(r), _ptr(rev_j), _ptr(z),
                                     int(seed) & (2 ** 64 - 1), int(sweep), _ptr(w_out), _stream(dev)),
           "nngp_gibbs_w_color")


def gibbs_w_apply(rows: torch.Tensor, w_src: torch.Tensor, B: torch.Tensor, w: torch.Tensor, r: torch.Tensor,
                  rev_j: torch.Tensor, rev_k: torch.Tensor) -> None:
    """Replay other ranks' colour draws (nngp_gibbs_w_apply): rows int32 (k, 4) = (i, off[i],
    off[i + 1], src), w_src[src] the owner's new w_i."""
    dev = _require_gpu(rows, w_src, B, w, r, rev_j, rev_k)
    if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 4 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous int32 (k, 4) tensor")
    n, m = B.shape
    _check(load().nngp_gibbs_w_apply(_ptr(rows), rows.shape[0], _ptr(w_src), _ptr(B), n, m, _ptr(w), _ptr(r),
                                     _ptr(rev_j), _ptr(rev_k), _stream(dev)), "nngp_gibbs_w_apply")


def _check_noise_w(noise_w: Optional[torch.Tensor], n: int) -> None:
    if noise_w is not None and (noise_w.dtype != torch.float64 or noise_w.shape != (n,)
                                or not noise_w.is_contiguous()):
        raise ValueError(f"noise_w must be a contiguous float64 ({n},) tensor")


def _check_member_rows(rows: torch.Tensor, co, n: int, n_entries: int) -> None:
    """The colour kernels index w / r / the prep with each member row's location and reverse range unchecked:
    verify them once per rows tensor (0 <= location < n, 0 <= first <= end <= n_entries), and the colour
    offsets against the row count on every call."""
    if co.size and int(co[-1]) > rows.shape[0]:  # (negative offsets: refused by the C ABI)
        raise ValueError(f"colour offsets reach past the {rows.shape[0]} member rows")
    key = (n, n_entries, rows.data_ptr())
    if getattr(rows, "_nngp_bounds", None) == key:
        return
    if rows.shape[0]:
        i, e0, e1 = rows[:, 0], rows[:, 1], rows[:, 2]
        if bool(((i < 0) | (i >= n) | (e0 < 0) | (e1 < e0) | (e1 > n_entries)).any()):
            raise ValueError("member_rows hold a location outside [0, n) or a reverse range outside the entries: "
                             "build them with gibbs_member_rows(members, off) for this field")
    rows._nngp_bounds = key


def gibbs_member_rows(members: torch.Tensor, off: torch.Tensor) -> torch.Tensor:
    """int32 (n, 4) rows (location, first / end reverse entry, 0) of the colour-ordered
    ``members`` (nngp_gibbs_member_rows): build once per colouring, pass to :func:`gibbs_w_sweep`."""
    dev = _require_gpu(members, off)
    if members.dtype != torch.int32 or off.dtype != torch.int32 or members.dim() != 1:
        raise ValueError("members and off must be int32, members 1-D")
    members, off = members.contiguous(), off.contiguous()
    rows = torch.empty((members.shape[0], 4), dtype=torch.int32, device=dev)
    _check(load().nngp_gibbs_member_rows(_ptr(members), members.shape[0], _ptr(off), _ptr(rows), _stream(dev)),
           "nngp_gibbs_member_rows")
    return rows


def gibbs_w_sweep(members: torch.Tensor, color_off_host, prep: torch.Tensor, m: int, sigma2: float,
                  tau2: float, yres: torch.Tensor, w: torch.Tensor, r: torch.Tensor, off: torch.Tensor,
                  rev_j: torch.Tensor, seed: int, sweep: int, z: Optional[torch.Tensor] = None,
                  noise_w: Optional[torch.Tensor] = None, member_rows: Optional[torch.Tensor] = None) -> None:
    """One colour-ordered sweep of w_i | rest, in place on w and r (see include/nngp.h);
    ``prep`` from :func:`gibbs_prepare` for the current B / Ft; ``noise_w`` (n,) optional
    weights h_i (noise variance tau2 / h_i); ``member_rows`` from :func:`gibbs_member_rows`
    (built from ``members`` and ``off`` here when not given)."""
    import numpy as np

    dev = _require_gpu(members, prep, yres, w, r, off, rev_j, z, noise_w, member_rows)
    _check_noise_w(noise_w, w.shape[0])
    if member_rows is None:
        member_rows = gibbs_member_rows(members, off)
    elif member_rows.dtype != torch.int32 or tuple(member_rows.shape) != (members.shape[0], 4) \
            or not member_rows.is_contiguous():
        raise ValueError("member_rows must be a contiguous int32 (n, 4) tensor from gibbs_member_rows")
    co = np.ascontiguousarray(color_off_host, dtype=np.int32)
    n = w.shape[0]
    _check_member_rows(member_rows, co, n, 0 if rev_j is None else rev_j.numel())
    _check(load().nngp_gibbs_w_sweep(_ptr(member_rows), co.ctypes.data, len(co) - 1, _ptr(prep), n, int(m),
                                     float(sigma2), float(tau2), _ptr(yres), _ptr(noise_w), _ptr(w), _ptr(r),
                                     _ptr(rev_j),
                                     _ptr(z), int(seed) & (2 ** 64 - 1), int(sweep), _stream(dev)),
           "nngp_gibbs_w_sweep")


def gibbs_w_sweep_tiles(plan, prep: torch.Tensor, m: int, sigma2: float, tau2: float, yres: torch.Tensor,
                        w: torch.Tensor, r: torch.Tensor, off: torch.Tensor, z: torch.Tensor,
                        noise_w: Optional[torch.Tensor] = None, rev_j: Optional[torch.Tensor] = None) -> None:
    """The tiled colour sweep (nngp_gibbs_w_sweep_tiles) over a :class:`pynngp_amd.gibbs_tiles.TilePlan`: one
    launch per phase, each tile's footprint of r in LDS; in place on w and r; ``z`` the normals
    (:func:`gibbs_normals`).  The order is the plan's (level, phase, colour) -- its ``effective_colors`` as a
    colouring.  The plan must be contiguous (its node order is the storage order: ``plan.contiguous``;
    :func:`pynngp_amd.gibbs_tiles.contiguous_plan` / SeqNNGP(sweep="tiled") arrange it).  A plan built with
    coarse="colour" sweeps its coarse nodes after the tiles, one launch per colour (:func:`gibbs_w_sweep`,
    which needs ``rev_j``)."""
    dev = _require_gpu(prep, yres, w, r, off, z, noise_w, plan.tinfo)
    _check_noise_w(noise_w, w.shape[0])
    if not plan.contiguous:
        raise ValueError("the tiled sweep needs a contiguous tile plan (tile t's nodes = storage rows [n0, n1)): "
                         "store the field in plan.tnodes order and rebuild the plan there")
    if plan.tnodes.numel() != w.shape[0]:
        raise ValueError(f"the tile plan covers {plan.tnodes.numel()} nodes, the field has {w.shape[0]}")
    key = (w.shape[0], off.data_ptr())
    if getattr(plan, "_bounds_ok", None) != key:  # what the kernel indexes unchecked, once per plan and field
        from .gibbs_tiles import validate_launch_bounds

        validate_launch_bounds(plan, off, w.shape[0])
        plan._bounds_ok = key
    tiles, poff, plds = plan.launch_arrays()
    _check(load().nngp_gibbs_w_sweep_tiles(_ptr(tiles), poff.ctypes.data, plds.ctypes.data, len(plds),
                                           _ptr(plan.tinfo), _ptr(plan.tstep), int(plan.ecap), _ptr(plan.tfp),
                                           _ptr(off), _ptr(plan.rev_loc), _ptr(prep), w.shape[0], int(m),
                                           int(plan.rev_loc.numel()), float(sigma2), float(tau2), _ptr(yres),
                                           _ptr(noise_w), _ptr(w), _ptr(r), _ptr(z), _stream(dev)),
           "nngp_gibbs_w_sweep_tiles")
    if plan.coarse_members is not None and plan.coarse_members.numel() > 0:
        if rev_j is None:
            raise ValueError("a tile plan with coarse nodes swept per colour needs rev_j")
        if getattr(plan, "_coarse_rows", None) is None:
            plan._coarse_rows = gibbs_member_rows(plan.coarse_members, off)
        gibbs_w_sweep(plan.coarse_members, plan.coarse_color_off, prep, m, sigma2, tau2, yres, w, r, off, rev_j, 0, 0,
                      z=z, noise_w=noise_w, member_rows=plan._coarse_rows)


def gibbs_w_sweep_chains(member_rows: torch.Tensor, color_off_host, preps, m: int, sigma2s, tau2s, yres, w, r,
                         rev_j: torch.Tensor, z, noise_w: Optional[torch.Tensor] = None) -> None:
    """:func:`gibbs_w_sweep` for up to 8 independent chains of one field in ONE launch per colour
    (nngp_gibbs_w_sweep_chains): ``member_rows`` / colours / ``rev_j`` / ``noise_w`` shared, per chain
    lists of ``preps``, ``sigma2s``, ``tau2s``, ``yres`` and given normals ``z``; ``w`` and ``r`` either
    per-chain lists of (n,) vectors or two contiguous (n, C) tensors holding the chains interleaved
    (nngp_gibbs_w_sweep_chains_il: one sector per scattered access for all chains).  Chain c's result is
    bit-identical to :func:`gibbs_w_sweep` on its own arguments with its ``z``."""
    import numpy as np

    C = len(preps)
    il = isinstance(w, torch.Tensor)
    if il != isinstance(r, torch.Tensor):
        raise ValueError("w and r: both per-chain lists or both (n, C) tensors")
    per = (sigma2s, tau2s, yres, z) if il else (sigma2s, tau2s, yres, w, r, z)
    if not 1 <= C <= 8 or not all(len(v) == C for v in per):
        raise ValueError("1..8 chains, one entry per chain in every list")
    n = w.shape[0] if il else w[0].shape[0]
    if il:
        for t in (w, r):
            if t.dtype != torch.float64 or tuple(t.shape) != (n, C) or not t.is_contiguous():
                raise ValueError(f"interleaved w / r must be contiguous float64 ({n}, {C})")
    vecs = list(yres) + list(z) + ([] if il else list(w) + list(r))
    for t in vecs:
        if t.dtype != torch.float64 or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"per-chain vectors must be contiguous float64 ({n},)")
    if member_rows.dtype != torch.int32 or member_rows.dim() != 2 or member_rows.shape[1] != 4 \
            or not member_rows.is_contiguous():
        raise ValueError("member_rows must be a contiguous int32 (n, 4) tensor from gibbs_member_rows")
    dev = _require_gpu(member_rows, rev_j, noise_w, *preps, *vecs, *((w, r) if il else ()))
    _check_noise_w(noise_w, n)
    co = np.ascontiguousarray(color_off_host, dtype=np.int32)
    _check_member_rows(member_rows, co, n, 0 if rev_j is None else rev_j.numel())
    P = ctypes.c_void_p * C
    D = ctypes.c_double * C
    head = (_ptr(member_rows), co.ctypes.data, len(co) - 1, C, P(*[_ptr(t) for t in preps]), n, int(m),
            D(*map(float, sigma2s)), D(*map(float, tau2s)), P(*[_ptr(t) for t in yres]), _ptr(noise_w))
    tail = (_ptr(rev_j), P(*[_ptr(t) for t in z]), _stream(dev))
    if il:
        _check(load().nngp_gibbs_w_sweep_chains_il(*head, _ptr(w), _ptr(r), *tail), "nngp_gibbs_w_sweep_chains_il")
    else:
        _check(load().nngp_gibbs_w_sweep_chains(*head, P(*[_ptr(t) for t in w]), P(*[_ptr(t) for t in r]), *tail),
               "nngp_gibbs_w_sweep_chains")


def gibbs_normals(z: torch.Tensor, seed: int, sweep: int) -> torch.Tensor:
    """Fill z (float64 (n,)) with the sweep's Philox normals (nngp_gibbs_normals)."""
    dev = _require_gpu(z)
    if z.dtype != torch.float64 or z.dim() != 1:
        raise ValueError("z must be float64 (n,)")
    _check(load().nngp_gibbs_normals(z.shape[0], int(seed) & (2 ** 64 - 1), int(sweep), _ptr(z), _stream(dev)),
           "nngp_gibbs_normals")
    return z


def gibbs_stats(r: torch.Tensor, Ft: torch.Tensor, yres: torch.Tensor, y: torch.Tensor, X: Optional[torch.Tensor],
                w: torch.Tensor, out: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None, noise_w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[sum r^2/Ft, sum h (yres - w)^2, X^T H (y - w)...] as a float64 device tensor (2 + p,);
    h = ``noise_w`` (n,) or 1."""
    dev = _require_gpu(r, Ft, yres, y, X, w, noise_w)
    _check_noise_w(noise_w, r.shape[0])
    n = r.shape[0]
    p = 0 if X is None else X.shape[1]
    lib = load()
    out = torch.empty(2 + p, dtype=torch.float64, device=dev) if out is None else out
    need = lib.nngp_gibbs_stats_workspace_bytes(n, p)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    _check(lib.nngp_gibbs_stats(n, _ptr(r), _ptr(Ft), _ptr(yres), _ptr(y), _ptr(X), p, _ptr(w), _ptr(noise_w), _ptr(out),
                                _ptr(workspace), workspace.numel(), _stream(dev)), "nngp_gibbs_stats")
    return out


# ---------------------------------------------------------------------------- Polya-Gamma draws (binomial model)
def check_trials(trials) -> None:
    """Refuse trials outside [0, PG_MAX_TRIALS] before any launch (one host synchronisation for a device tensor)."""
    if trials.numel() and (int(trials.min()) < 0 or int(trials.max()) > PG_MAX_TRIALS):
        raise ValueError(f"trials must lie in [0, {PG_MAX_TRIALS}] (got [{int(trials.min())}, {int(trials.max())}])")


def _pg_vec(t, n, name, dtype=torch.float64):
    if t.dtype != dtype or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} ({n},) tensor, got {t.dtype} {tuple(t.shape)}")


def _pg_sweep(sweep) -> int:
    if not 0 <= int(sweep) < 2 ** 40:
        raise ValueError("sweep (the iteration) must lie in [0, 2^40)")
    return int(sweep)


def polya_gamma(trials: torch.Tensor, c: torch.Tensor, seed: int = 0, sweep: int = 0,
                omega: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None, checked: bool = False):
    """omega[i] ~ PG(trials[i], c[i]) (nngp_polya_gamma): returns (omega, status), status an int32 (1,) device
    tensor holding 0 (clean) or the smallest index + 1 whose draw is NaN (non-finite c, or a loop cap).
    ``checked``: the caller has range-checked ``trials`` already."""
    if not (trials.is_cuda and c.is_cuda):
        raise NotImplementedError("pynngp_amd has no CPU path: polya_gamma needs ROCm GPU tensors")
    dev = _require_gpu(trials, c, omega, status)
    n = trials.shape[0] if trials.dim() == 1 else -1
    _pg_vec(trials, n, "trials", torch.int32)
    _pg_vec(c, n, "c")
    if not checked:
        check_trials(trials)
    omega = torch.empty(n, dtype=torch.float64, device=dev) if omega is None else omega
    status = torch.empty(1, dtype=torch.int32, device=dev) if status is None else status
    _pg_vec(omega, n, "omega")
    _pg_vec(status, 1, "status", torch.int32)
    _check(load().nngp_polya_gamma(n, _ptr(trials), _ptr(c), int(seed) & (2 ** 64 - 1), _pg_sweep(sweep), _ptr(omega),
                                   _ptr(status), _stream(dev)), "nngp_polya_gamma")
    return omega, status


def gibbs_pg_update(trials: torch.Tensor, kappa: torch.Tensor, xb: torch.Tensor, w: torch.Tensor, seed: int,
                    sweep: int, omega: Optional[torch.Tensor] = None, yres: Optional[torch.Tensor] = None,
                    status: Optional[torch.Tensor] = None, checked: bool = False):
    """The binomial sampler's fused draw (nngp_gibbs_pg_update): omega ~ PG(trials, xb + w) and
    yres = kappa / omega - xb (both 0 where trials = 0); returns (omega, yres, status)."""
    if not (trials.is_cuda and kappa.is_cuda and xb.is_cuda and w.is_cuda):
        raise NotImplementedError("pynngp_amd has no CPU path: gibbs_pg_update needs ROCm GPU tensors")
    dev = _require_gpu(trials, kappa, xb, w, omega, yres, status)
    n = trials.shape[0] if trials.dim() == 1 else -1
    _pg_vec(trials, n, "trials", torch.int32)
    for t, name in ((kappa, "kappa"), (xb, "xb"), (w, "w")):
        _pg_vec(t, n, name)
    if not checked:
        check_trials(trials)
    omega = torch.empty(n, dtype=torch.float64, device=dev) if omega is None else omega
    yres = torch.empty(n, dtype=torch.float64, device=dev) if yres is None else yres
    status = torch.empty(1, dtype=torch.int32, device=dev) if status is None else status
    _pg_vec(omega, n, "omega")
    _pg_vec(yres, n, "yres")
    _pg_vec(status, 1, "status", torch.int32)
    _check(load().nngp_gibbs_pg_update(n, _ptr(trials), _ptr(kappa), _ptr(xb), _ptr(w), int(seed) & (2 ** 64 - 1),
                                       _pg_sweep(sweep), _ptr(omega), _ptr(yres), _ptr(status), _stream(dev)),
           "nngp_gibbs_pg_update")
    return omega, yres, status


# ---------------------------------------------------------------------------- binomial latent posterior (Laplace)
def binomial_newton_step(trials: torch.Tensor, successes: torch.Tensor, offset: torch.Tensor, w: torch.Tensor,
                         d: Optional[torch.Tensor] = None, rhs: Optional[torch.Tensor] = None,
                         g: Optional[torch.Tensor] = None, partials: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None):
    """One Newton step's link quantities per node (nngp_binomial_newton_step): ``(d, rhs, g, partials)`` with d = W =
    b p (1 - p), g = s - b p, rhs = W w + g at eta = offset + w, and partials (4,) on the device = (sum of the
    log-likelihood terms, max |g|, first node with a non-finite eta + 1 or 0, first node with negative trials + 1 or
    0).  Faults are data: nothing is read back here (:func:`binomial_check_partials` does that)."""
    if not (trials.is_cuda and successes.is_cuda and offset.is_cuda and w.is_cuda):
        raise NotImplementedError("pynngp_amd has no CPU path: binomial_newton_step needs ROCm GPU tensors")
    dev = _require_gpu(trials, successes, offset, w, d, rhs, g, partials)
    n = trials.shape[0] if trials.dim() == 1 else -1
    _pg_vec(trials, n, "trials", torch.int32)
    for t, name in ((successes, "successes"), (offset, "offset"), (w, "w")):
        _pg_vec(t, n, name)
    d = torch.empty(n, dtype=torch.float64, device=dev) if d is None else d
    rhs = torch.empty(n, dtype=torch.float64, device=dev) if rhs is None else rhs
    g = torch.empty(n, dtype=torch.float64, device=dev) if g is None else g
    partials = torch.empty(4, dtype=torch.float64, device=dev) if partials is None else partials
    for t, name in ((d, "d"), (rhs, "rhs"), (g, "g")):
        _pg_vec(t, n, name)
    _pg_vec(partials, 4, "partials")
    lib = load()
    need = lib.nngp_binomial_newton_step_workspace_bytes(n)
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    _check(lib.nngp_binomial_newton_step(n, _ptr(trials), _ptr(successes), _ptr(offset), _ptr(w), _ptr(d), _ptr(rhs),
                                         _ptr(g), _ptr(partials), _ptr(workspace), workspace.numel(), _stream(dev)),
           "nngp_binomial_newton_step")
    return d, rhs, g, partials


def binomial_check_partials(partials_host) -> Tuple[int, int]:
    """``(first_nonfinite, first_negative_trials)`` of host-resident partials of :func:`binomial_newton_step`
    (nngp_binomial_check_partials), -1 = none."""
    p = (ctypes.c_double * 4)(*[float(v) for v in partials_host])
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    load().nngp_binomial_check_partials(ctypes.cast(p, ctypes.c_void_p), ctypes.cast(ctypes.byref(a), ctypes.c_void_p),
                                        ctypes.cast(ctypes.byref(b), ctypes.c_void_p))
    return int(a.value), int(b.value)


def logistic_normal(mu: torch.Tensor, s: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = E[logistic(mu[i] + s[i] Z)], Z ~ N(0, 1) (nngp_logistic_normal; s = 0: logistic(mu))."""
    if not (mu.is_cuda and s.is_cuda):
        raise NotImplementedError("pynngp_amd has no CPU path: logistic_normal needs ROCm GPU tensors")
    dev = _require_gpu(mu, s, out)
    n = mu.shape[0] if mu.dim() == 1 else -1
    _pg_vec(mu, n, "mu")
    _pg_vec(s, n, "s")
    out = torch.empty(n, dtype=torch.float64, device=dev) if out is None else out
    _pg_vec(out, n, "out")
    _check(load().nngp_logistic_normal(n, _ptr(mu), _ptr(s), _ptr(out), _stream(dev)), "nngp_logistic_normal")
    return out


def gibbs_pg_stats(r: torch.Tensor, Ft: torch.Tensor, omega: torch.Tensor, kappa: torch.Tensor,
                   X: Optional[torch.Tensor], w: torch.Tensor, out: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[sum r^2/Ft, upper triangle of X' Omega X (row by row), X'(kappa - Omega w)] as a float64 device tensor
    (1 + p (p + 1) / 2 + p,) (nngp_gibbs_pg_stats; fixed-order folds: the same bits on every call)."""
    dev = _require_gpu(r, Ft, omega, kappa, X, w, out, workspace)
    n = r.shape[0] if r.dim() == 1 else -1
    for t, name in ((r, "r"), (Ft, "Ft"), (omega, "omega"), (kappa, "kappa"), (w, "w")):
        _pg_vec(t, n, name)
    p = 0 if X is None else X.shape[1]
    if X is not None and (X.dtype != torch.float64 or tuple(X.shape) != (n, p) or not X.is_contiguous()):
        raise ValueError(f"X must be a contiguous float64 ({n}, p) tensor")
    nv = 1 + p * (p + 1) // 2 + p
    lib = load()
    need = lib.nngp_gibbs_pg_stats_workspace_bytes(n, p)
    if need == 0:
        raise ValueError(f"gibbs_pg_stats needs n >= 1 and 0 <= p <= 62 (n={n}, p={p})")
    out = torch.empty(nv, dtype=torch.float64, device=dev) if out is None else out
    _pg_vec(out, nv, "out")
    if workspace is None or workspace.numel() < need:
        workspace = _workspace(need, dev)
    _check(lib.nngp_gibbs_pg_stats(n, _ptr(r), _ptr(Ft), _ptr(omega), _ptr(kappa), _ptr(X), p, _ptr(w), _ptr(out),
                                   _ptr(workspace), _stream(dev)), "nngp_gibbs_pg_stats")
    return out


# ---------------------------------------------------------------------------- latent-field posterior
# (include/nngp.h: "Latent-field posterior at fixed theta" and "... on a reference set")
class _LatentCall:
    """The arguments of one latent call, checked (raw pointers below: a short array must never reach a kernel), and
    the call itself.  ``geom`` = (nbr, B, off, rev_j, rev_k, prep) of an n-node DAG whose first ``n_s`` nodes are
    the reference set; ``n_s`` None: an S = T entry point (n_s = n, and the C call takes no n_s).  ``vectors``:
    name -> (tensor, rows), rows one of "s" (the n_s reference nodes), "n" (all nodes) or "l" (the leaves), with a
    "?" where the tensor may be None; each is float64 (rows, nrhs) with one nrhs in [1, LATENT_MAX_RHS], or
    (rows,) when not ``batched`` (the C call then takes no nrhs).  ``d``: (n,) or None.  Every ValueError comes
    before any device work."""

    def __init__(self, geom, n_s, sigma2, d, batched=True, **vectors):
        nbr, B, off, rev_j, rev_k, prep = geom
        if nbr.dtype != torch.int32 or nbr.dim() != 2:
            raise ValueError(f"nbr must be int32 (n, m), got {nbr.dtype} {tuple(nbr.shape)}")
        n, m = nbr.shape
        self.ref = n_s is not None
        n_s = int(n_s) if self.ref else n
        if not 0 <= n_s <= n:
            raise ValueError(f"need 0 <= n_s <= n = {n}, got n_s={n_s}")
        if not 1 <= m <= MAX_M:
            raise ValueError(f"m={m} outside [1, {MAX_M}]")
        if B.dtype != torch.float64 or tuple(B.shape) != (n, m):
            raise ValueError(f"B must be float64 ({n}, {m}), got {B.dtype} {tuple(B.shape)}")
        if off.dtype != torch.int32 or tuple(off.shape) != (n + 1,):
            raise ValueError(f"off must be int32 ({n + 1},)")
        for name, t in (("rev_j", rev_j), ("rev_k", rev_k)):
            if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < n * m:
                raise ValueError(f"{name} must be int32 with at least n * m = {n * m} entries")
        rows = {"s": n_s, "n": n, "l": n - n_s}
        nrhs = None if batched else 1
        for name, (t, kind) in vectors.items():
            if t is None:
                if not kind.endswith("?"):
                    raise ValueError(f"{name} is needed")
                continue
            cols = nrhs if nrhs is not None else t.shape[1] if t.dim() == 2 else "nrhs"
            shape = (rows[kind[0]], cols) if batched else (rows[kind[0]],)
            if t.dtype != torch.float64 or tuple(t.shape) != shape:
                raise ValueError(f"{name} must be float64 {shape}, got {t.dtype} {tuple(t.shape)}")
            if nrhs is None:
                nrhs = cols
                if not 1 <= nrhs <= LATENT_MAX_RHS:
                    raise ValueError(f"nrhs={nrhs} outside [1, {LATENT_MAX_RHS}]")
        if d is not None and (d.dtype != torch.float64 or tuple(d.shape) != (n,)):
            raise ValueError(f"d must be float64 ({n},), got {d.dtype} {tuple(d.shape)}")
        if d is not None and "z2" in vectors and vectors["z2"][0] is None:
            raise ValueError("z2 is needed when d is given")
        tensors = geom + (d,) + tuple(t for t, _ in vectors.values())
        if not all(t.is_contiguous() for t in tensors if t is not None):
            raise ValueError("the operator's arguments must be contiguous")
        self.dev = _require_gpu(*tensors)
        if prep.dtype != torch.uint8 or prep.numel() < load().nngp_gibbs_prep_bytes(n, m):
            raise ValueError("prep must be the uint8 buffer of gibbs_prepare for these factors")
        self.geom, self.sigma2, self.d, self.batched, self.rows = geom, float(sigma2), d, batched, rows
        self.n, self.n_s, self.m, self.nrhs = n, n_s, m, nrhs

    def empty(self, kind):
        """A result vector on the rows ``kind``."""
        shape = (self.rows[kind], self.nrhs) if self.batched else (self.rows[kind],)
        return torch.empty(shape, dtype=torch.float64, device=self.dev)

    def __call__(self, symbol, args, ws_symbol=None, workspace=None, trace=None):
        """``symbol``(geometry, n[, n_s], m, sigma2, d[, nrhs], *args[, workspace, its bytes][, trace, its length],
        stream); tensors among ``args`` go as pointers.  ``ws_symbol``: the call takes a workspace of that many
        bytes, made here unless the caller's is large enough.  ``trace``: the call takes a trace argument -- a
        checked (nrhs, trace_len, 2) tensor (:meth:`check_trace`), or ``()`` for the NULL trace."""
        lib = load()
        sizes = (self.n, self.n_s) if self.ref else (self.n,)
        k = (self.nrhs,) if self.batched else ()
        argv = [_ptr(t) for t in self.geom] + [*sizes, self.m, self.sigma2, _ptr(self.d), *k]
        argv += [_ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
        if ws_symbol is not None:
            need = getattr(lib, ws_symbol)(*sizes, *(k or ((1,) if self.ref else ())))
            if workspace is None or workspace.numel() < need:
                workspace = _workspace(need, self.dev)
            argv += [_ptr(workspace), workspace.numel()]
        if trace is not None:
            argv += [_ptr(trace), trace.shape[1]] if isinstance(trace, torch.Tensor) else [None, 0]
        _check(getattr(lib, symbol)(*argv, _stream(self.dev)), symbol)

    def check_trace(self, trace, max_iter):
        """A CG trace: contiguous float64 (nrhs, trace_len >= max_iter, 2) on the call's device."""
        if (not isinstance(trace, torch.Tensor) or trace.dtype != torch.float64 or trace.dim() != 3
                or trace.shape[0] != self.nrhs or trace.shape[2] != 2 or not trace.is_contiguous()):
            raise ValueError(f"trace must be a contiguous float64 ({self.nrhs}, trace_len, 2) tensor")
        if trace.shape[1] < max_iter:
            raise ValueError(f"trace_len={trace.shape[1]} is below max_iter={max_iter}")
        if trace.device != self.dev:
            raise ValueError(f"trace must be on {self.dev}, got {trace.device}")
        return trace


def _latent_apply(c, symbol, ws_symbol, x, out, workspace):
    out = c.empty("s") if out is None else out
    c(symbol, (x, out), ws_symbol, workspace)
    return out


def _latent_sqrt_t_apply(c, symbol, ws_symbol, z1, z2, out, workspace):
    out = c.empty("s") if out is None else out
    c(symbol, (z1, z2, out), ws_symbol, workspace)
    return out


def _latent_cg(c, symbol, ws_symbol, b, x, rtol, max_iter, check_every, workspace, trace=None):
    info = np.zeros((c.nrhs, 4), dtype=np.float64)
    c(symbol, (b, x, float(rtol), int(max_iter), int(check_every), info.ctypes.data_as(ctypes.c_void_p)), ws_symbol,
      workspace, trace)
    return x, info


def precision_apply(nbr: torch.Tensor, B: torch.Tensor, off: torch.Tensor, rev_j: torch.Tensor, rev_k: torch.Tensor,
                    prep: torch.Tensor, sigma2: float, x: torch.Tensor, d: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = [(I - B)^T (sigma2 F)^-1 (I - B) + diag(d)] x (nngp_precision_apply): ``prep`` from
    :func:`gibbs_prepare` of the unit-variance (B, F), the reverse lists from :func:`reverse_neighbors`;
    ``d`` None = the prior precision alone.  Bit-reproducible; stream-ordered, no host synchronisation."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), None, sigma2, d, False, x=(x, "s"), out=(out, "s?"))
    return _latent_apply(c, "nngp_precision_apply", "nngp_precision_workspace_bytes", x, out, workspace)


def precision_sqrt_t_apply(nbr: torch.Tensor, B: torch.Tensor, off: torch.Tensor, rev_j: torch.Tensor,
                           rev_k: torch.Tensor, prep: torch.Tensor, sigma2: float, z1: torch.Tensor,
                           z2: Optional[torch.Tensor] = None, d: Optional[torch.Tensor] = None,
                           out: Optional[torch.Tensor] = None,
                           workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (I - B)^T (sigma2 F)^-1/2 z1 + sqrt(d) z2 (nngp_precision_sqrt_t_apply): Cov(out) = A for standard
    normal z1, z2 -- the perturbation of exact posterior draws."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), None, sigma2, d, False, z1=(z1, "n"), z2=(z2, "s?"),
                    out=(out, "s?"))
    return _latent_sqrt_t_apply(c, "nngp_precision_sqrt_t_apply", "nngp_precision_workspace_bytes", z1, z2, out,
                                workspace)


def latent_cg(nbr: torch.Tensor, B: torch.Tensor, off: torch.Tensor, rev_j: torch.Tensor, rev_k: torch.Tensor,
              prep: torch.Tensor, sigma2: float, b: torch.Tensor, x: torch.Tensor, d: Optional[torch.Tensor] = None,
              rtol: float = 1e-8, max_iter: int = 1000, check_every: int = 8,
              workspace: Optional[torch.Tensor] = None):
    """Jacobi-preconditioned CG for A x = b in place on ``x`` (its start; nngp_latent_cg).  Returns
    ``(x, info)``, info = [iterations, converged (1 / 0 / -1 breakdown), |r|^2, |b|^2] as host floats.
    Synchronises the stream once per ``check_every`` iterations."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), None, sigma2, d, False, b=(b, "s"), x=(x, "s"))
    x, info = _latent_cg(c, "nngp_latent_cg", "nngp_latent_cg_workspace_bytes", b, x, rtol, max_iter, check_every,
                         workspace)
    return x, [float(v) for v in info[0]]


def precision_apply_batch(nbr: torch.Tensor, B: torch.Tensor, off: torch.Tensor, rev_j: torch.Tensor,
                          rev_k: torch.Tensor, prep: torch.Tensor, sigma2: float, x: torch.Tensor,
                          d: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = A x for ``x`` (n, nrhs), 1 <= nrhs <= LATENT_MAX_RHS (nngp_precision_apply_batch): every index and
    coefficient is read once for all columns.  Column c is bit-identical to :func:`precision_apply` on it."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), None, sigma2, d, x=(x, "s"), out=(out, "s?"))
    return _latent_apply(c, "nngp_precision_apply_batch", "nngp_precision_batch_workspace_bytes", x, out, workspace)


def precision_sqrt_t_apply_batch(nbr: torch.Tensor, B: torch.Tensor, off: torch.Tensor, rev_j: torch.Tensor,
                                 rev_k: torch.Tensor, prep: torch.Tensor, sigma2: float, z1: torch.Tensor,
                                 z2: Optional[torch.Tensor] = None, d: Optional[torch.Tensor] = None,
                                 out: Optional[torch.Tensor] = None,
                                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (I - B)^T (sigma2 F)^-1/2 z1 + sqrt(d) z2 for ``z1`` / ``z2`` (n, nrhs)
    (nngp_precision_sqrt_t_apply_batch); column c is bit-identical to :func:`precision_sqrt_t_apply` on it."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), None, sigma2, d, z1=(z1, "n"), z2=(z2, "s?"), out=(out, "s?"))
    return _latent_sqrt_t_apply(c, "nngp_precision_sqrt_t_apply_batch", "nngp_precision_batch_workspace_bytes", z1,
                                z2, out, workspace)


def latent_cg_batch(nbr: torch.Tensor, B: torch.Tensor, off: torch.Tensor, rev_j: torch.Tensor, rev_k: torch.Tensor,
                    prep: torch.Tensor, sigma2: float, b: torch.Tensor, x: torch.Tensor,
                    d: Optional[torch.Tensor] = None, rtol: float = 1e-8, max_iter: int = 1000, check_every: int = 8,
                    workspace: Optional[torch.Tensor] = None):
    """nrhs Jacobi-PCG solves in lock step, in place on ``x`` (n, nrhs) (its start; nngp_latent_cg_batch).
    Returns ``(x, info)``, info a numpy (nrhs, 4) array whose row c is :func:`latent_cg`'s info of column c;
    column c of ``x`` is bit-identical to that single solve.  Synchronises once per ``check_every`` iterations."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), None, sigma2, d, b=(b, "s"), x=(x, "s"))
    return _latent_cg(c, "nngp_latent_cg_batch", "nngp_latent_cg_batch_workspace_bytes", b, x, rtol, max_iter,
                      check_every, workspace)


def precision_diag(prep: torch.Tensor, n: int, m: int, sigma2: float, d: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """diag(A) = d + (invF + P) / sigma2 from the ``prep`` buffer (nngp_precision_diag): the expression whose
    reciprocal preconditions the CG.  (No DAG is passed, so its few checks are its own.)"""
    n, m = int(n), int(m)
    if n < 0 or not 1 <= m <= MAX_M:
        raise ValueError(f"need n >= 0 and 1 <= m <= {MAX_M}, got n={n}, m={m}")
    for t in (d, out):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != (n,) or not t.is_contiguous()):
            raise ValueError(f"d and out must be contiguous float64 ({n},)")
    dev = _require_gpu(prep, d, out)
    lib = load()
    if prep.dtype != torch.uint8 or not prep.is_contiguous() or prep.numel() < lib.nngp_gibbs_prep_bytes(n, m):
        raise ValueError("prep must be the uint8 buffer of gibbs_prepare for these factors")
    out = torch.empty(n, dtype=torch.float64, device=dev) if out is None else out
    _check(lib.nngp_precision_diag(_ptr(prep), n, m, float(sigma2), _ptr(d), _ptr(out), _stream(dev)),
           "nngp_precision_diag")
    return out


def precision_ref_apply_batch(nbr, B, off, rev_j, rev_k, prep, n_s: int, sigma2: float, x: torch.Tensor,
                              d: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                              workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = A_S x for ``x`` (n_s, nrhs) on the n-node DAG whose first ``n_s`` nodes are the reference set
    (nngp_precision_ref_apply_batch): A_S = (I - B_S)^T f_S (I - B_S) + d_S + B_L^T g B_L, the leaves integrated
    out.  ``d`` (n,) or None.  With n_s = n it equals :func:`precision_apply_batch` bit for bit."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), n_s, sigma2, d, x=(x, "s"), out=(out, "s?"))
    return _latent_apply(c, "nngp_precision_ref_apply_batch", "nngp_precision_ref_batch_workspace_bytes", x, out,
                         workspace)


def precision_ref_sqrt_t_apply_batch(nbr, B, off, rev_j, rev_k, prep, n_s: int, sigma2: float, z1: torch.Tensor,
                                     z2: Optional[torch.Tensor] = None, d: Optional[torch.Tensor] = None,
                                     out: Optional[torch.Tensor] = None,
                                     workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (n_s, nrhs) = (I - B_S)^T f_S^1/2 z1_S + B_L^T g^1/2 z1_L + d_S^1/2 z2 for ``z1`` (n, nrhs) and ``z2``
    (n_s, nrhs) (nngp_precision_ref_sqrt_t_apply_batch): Cov(out) = A_S for standard normals."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), n_s, sigma2, d, z1=(z1, "n"), z2=(z2, "s?"), out=(out, "s?"))
    return _latent_sqrt_t_apply(c, "nngp_precision_ref_sqrt_t_apply_batch",
                                "nngp_precision_ref_batch_workspace_bytes", z1, z2, out, workspace)


def precision_ref_fold_batch(nbr, B, off, rev_j, rev_k, prep, n_s: int, sigma2: float, v: torch.Tensor,
                             d: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                             workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (n_s, nrhs) = d_S v_S + B_L^T (g v_L) for ``v`` (n, nrhs) on all nodes (nngp_precision_ref_fold_batch):
    the right-hand side b_S of the mean when v is the centred response."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), n_s, sigma2, d, v=(v, "n"), out=(out, "s?"))
    return _latent_apply(c, "nngp_precision_ref_fold_batch", "nngp_precision_ref_batch_workspace_bytes", v, out,
                         workspace)


def precision_ref_diag(nbr, B, off, rev_j, rev_k, prep, n_s: int, sigma2: float, d: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """diag(A_S) (n_s,) (nngp_precision_ref_diag): d_i + f_i + sum over children of B^2 s, the expression whose
    reciprocal preconditions :func:`latent_ref_cg_batch`."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), n_s, sigma2, d, False, out=(out, "s?"))
    out = c.empty("s") if out is None else out
    c("nngp_precision_ref_diag", (out,), "nngp_precision_ref_batch_workspace_bytes", workspace)
    return out


def latent_ref_cg_batch(nbr, B, off, rev_j, rev_k, prep, n_s: int, sigma2: float, b: torch.Tensor, x: torch.Tensor,
                        d: Optional[torch.Tensor] = None, rtol: float = 1e-8, max_iter: int = 1000,
                        check_every: int = 8, workspace: Optional[torch.Tensor] = None):
    """nrhs Jacobi-PCG solves of A_S x = b in lock step, in place on ``x`` (n_s, nrhs) (nngp_latent_ref_cg_batch);
    ``(x, info)`` as :func:`latent_cg_batch`."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), n_s, sigma2, d, b=(b, "s"), x=(x, "s"))
    return _latent_cg(c, "nngp_latent_ref_cg_batch", "nngp_latent_ref_cg_batch_workspace_bytes", b, x, rtol,
                      max_iter, check_every, workspace)


def latent_ref_cg_batch_trace(nbr, B, off, rev_j, rev_k, prep, n_s: int, sigma2: float, b: torch.Tensor,
                              x: torch.Tensor, d: Optional[torch.Tensor] = None, rtol: float = 1e-8,
                              max_iter: int = 1000, check_every: int = 8, workspace: Optional[torch.Tensor] = None,
                              trace: Optional[torch.Tensor] = None):
    """:func:`latent_ref_cg_batch` that records each column's CG scalars (nngp_latent_ref_cg_batch_trace): ``trace``
    a device float64 (nrhs, trace_len >= max_iter, 2) tensor, written in place: ``trace[c, k] = (alpha_k, beta_k)``
    for every iteration k column c completed, nothing else (fill it with NaN to see which).  They are the Lanczos
    tridiagonal of M^-1/2 A_S M^-1/2 (:func:`pynngp_amd.lanczos_quadrature`).  ``trace`` None: the NULL trace, the
    same bits as :func:`latent_ref_cg_batch`.  n_s = n is S = T."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), n_s, sigma2, d, b=(b, "s"), x=(x, "s"))
    tr = () if trace is None else c.check_trace(trace, int(max_iter))
    return _latent_cg(c, "nngp_latent_ref_cg_batch_trace", "nngp_latent_ref_cg_batch_workspace_bytes", b, x, rtol,
                      max_iter, check_every, workspace, tr)


def latent_ref_leaves_batch(nbr, B, off, rev_j, rev_k, prep, n_s: int, sigma2: float, x: torch.Tensor,
                            v: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None,
                            d: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The leaves given ``x`` (n_s, nrhs) on the reference set (nngp_latent_ref_leaves_batch): out (n - n_s, nrhs) =
    (f a + d v) / (f + d) [+ z / sqrt(f + d)], a = B_L x; ``v``, ``z`` (n - n_s, nrhs) or None.  ``d`` None: out =
    a [+ z / sqrt(f)], kriging of the nrhs fields to unobserved leaves."""
    c = _LatentCall((nbr, B, off, rev_j, rev_k, prep), n_s, sigma2, d, x=(x, "s"), v=(v, "l?"), z=(z, "l?"),
                    out=(out, "l?"))
    out = c.empty("l") if out is None else out
    c("nngp_latent_ref_leaves_batch", (x, v, z, out))
    return out


def latent_rows_dot2_batch(nbr: torch.Tensor, B: torch.Tensor, dB: torch.Tensor, n_s: int, x: torch.Tensor):
    """Two weighted gathers over every node row in one pass (nngp_latent_rows_dot2_batch): ``(P, Q)``, both (n,
    nrhs), P[i, c] = sum_k B[i, k] x[nbr[i, k], c] and Q the same with ``dB``, for ``x`` (n_s, nrhs) on the
    reference nodes, 1 <= nrhs <= LATENT_MAX_RHS.  A slot that is -1 or names a node >= n_s adds exactly 0; column c
    is bit-identical to the one-column call on it."""
    if nbr.dtype != torch.int32 or nbr.dim() != 2 or not nbr.is_contiguous():
        raise ValueError(f"nbr must be contiguous int32 (n, m), got {nbr.dtype} {tuple(nbr.shape)}")
    n, m = nbr.shape
    n_s = int(n_s)
    if not 0 <= n_s <= n:
        raise ValueError(f"need 0 <= n_s <= n (got n_s={n_s}, n={n})")
    for t, name in ((B, "B"), (dB, "dB")):
        if t.dtype != torch.float64 or tuple(t.shape) != (n, m) or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous float64 ({n}, {m}), got {t.dtype} {tuple(t.shape)}")
    if (x.dtype != torch.float64 or x.dim() != 2 or x.shape[0] != n_s or not 1 <= x.shape[1] <= LATENT_MAX_RHS
            or not x.is_contiguous()):
        raise ValueError(f"x must be contiguous float64 ({n_s}, nrhs) with 1 <= nrhs <= {LATENT_MAX_RHS}, got "
                         f"{x.dtype} {tuple(x.shape)}")
    dev = _require_gpu(nbr, B, dB, x)
    nrhs = x.shape[1]
    p = torch.empty((n, nrhs), dtype=torch.float64, device=dev)
    q = torch.empty((n, nrhs), dtype=torch.float64, device=dev)
    _check(load().nngp_latent_rows_dot2_batch(_ptr(nbr), _ptr(B), _ptr(dB), n, n_s, m, nrhs, _ptr(x), _ptr(p), _ptr(q),
                                              _stream(dev)), "nngp_latent_rows_dot2_batch")
    return p, q


def whiten_gram(nbr: torch.Tensor, B: torch.Tensor, F: torch.Tensor, V: torch.Tensor, i0: int = 0,
                order: Optional[torch.Tensor] = None, Vq: Optional[torch.Tensor] = None, want_gram: bool = True,
                U: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """Whiten the columns ``V`` (n_points, ncol), 1 <= ncol <= WHITEN_MAX_COLS, by the stored factor and form their
    Gram matrix (nngp_whiten_gram): ``(U, G)`` with U (n_rows, ncol) = F^-1/2 (I - B) V and G (ncol, ncol) = U^T U
    (``want_gram=False``: G is None).  ``nbr`` / ``B`` / ``F`` as the sweeps wrote them; ``order``: the
    nngp_row_order layout when ``nbr`` holds the sorted rows; ``Vq`` (n_rows, ncol): the rows' own values for query
    rows against a reference set (default: S = T, row r is point ``i0 + r`` of V).  Column c of U is bit-identical
    to the one-column call and G[a, b] to the two-column call on (a, b)."""
    if nbr.dtype != torch.int32 or nbr.dim() != 2 or not nbr.is_contiguous():
        raise ValueError(f"nbr must be contiguous int32 (n_rows, m), got {nbr.dtype} {tuple(nbr.shape)}")
    n, m = nbr.shape
    if not 1 <= m <= MAX_M:
        raise ValueError(f"m={m} outside [1, {MAX_M}]")
    dev = _require_gpu(nbr, B, F, V, order, Vq, U, workspace)
    _check_out(B, "B", (n, m), dev)
    _check_out(F, "F", (n,), dev)
    if (V.dtype != torch.float64 or V.dim() != 2 or not 1 <= V.shape[1] <= WHITEN_MAX_COLS or not V.is_contiguous()
            or V.shape[0] < 1):
        raise ValueError(f"V must be contiguous float64 (n_points, ncol) with 1 <= ncol <= {WHITEN_MAX_COLS}, got "
                         f"{V.dtype} {tuple(V.shape)}")
    n_points, ncol = V.shape
    i0 = int(i0)
    _check_out(Vq, "Vq", (n, ncol), dev)
    if Vq is None and not 0 <= i0 <= n_points - n:
        raise ValueError(f"rows [{i0}, {i0 + n}) outside [0, {n_points})")
    if order is not None and (order.dtype != torch.int32 or tuple(order.shape) != (n,) or not order.is_contiguous()):
        raise ValueError(f"order must be contiguous int32 ({n},)")
    _check_out(U, "U", (n, ncol), dev)
    if U is None:
        U = torch.empty((n, ncol), dtype=torch.float64, device=dev)
    lib = load()
    need = lib.nngp_whiten_gram_workspace_bytes(n, ncol)
    ws = _workspace(need, dev) if workspace is None else workspace
    if ws.numel() < need:
        raise ValueError(f"workspace too small: {ws.numel()} < {need} bytes")
    G = torch.empty((ncol, ncol), dtype=torch.float64, device=dev) if want_gram else None
    _check(lib.nngp_whiten_gram(_ptr(nbr), _ptr(order), _ptr(B), _ptr(F), n, m, i0, n_points, ncol, _ptr(V), _ptr(Vq),
                                _ptr(U), _ptr(G), _ptr(ws), ws.numel(), _stream(dev)), "nngp_whiten_gram")
    return U, G


# -- solves with the NNGP factor (nngp_factor_*) ------------------------------------------------------------
class FactorSchedule:
    """One level schedule of :func:`factor_levels` with its device copies: ``level`` (n,) each row's level,
    ``rows`` (n,) the rows sorted by (level, index), ``level_off`` (depth + 1,) the levels' offsets into it (host
    numpy int32), ``rows_dev`` / ``level_off_dev`` the device tensors the solve reads, ``depth`` the level count."""

    def __init__(self, level, rows, level_off, device):
        self.level, self.rows, self.level_off = level, rows, level_off
        self.depth = level_off.shape[0] - 1
        self.rows_dev = torch.from_numpy(rows).to(device)
        self.level_off_dev = torch.from_numpy(level_off).to(device)

    def launch_counts(self, fuse_width: int):
        """``(wide levels, narrow runs)``: the launches of one solve at ``fuse_width`` (nngp_factor_launch_counts)."""
        wide, runs = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(load().nngp_factor_launch_counts(self.level_off.ctypes.data_as(ctypes.c_void_p), self.depth,
                                                int(fuse_width), ctypes.byref(wide), ctypes.byref(runs)),
               "nngp_factor_launch_counts")
        return int(wide.value), int(runs.value)

    def _args(self):
        return [_ptr(self.rows_dev), _ptr(self.level_off_dev), self.level_off.ctypes.data_as(ctypes.c_void_p),
                self.depth]


def factor_levels(nbr_host, trans: bool = False, device=None):
    """The level schedule of the factor's forward (``trans`` False) or transposed solve for the HOST neighbour array
    ``nbr_host`` (int32 (n, m), -1 padded; a slot that is negative or >= its row's index counts as -1)
    (nngp_factor_levels; no GPU).  Returns ``(level, rows, level_off)`` as numpy int32 arrays, or, with ``device``,
    a :class:`FactorSchedule` holding them and their device copies."""
    nb = np.ascontiguousarray(nbr_host, dtype=np.int32)
    if nb.ndim != 2:
        raise ValueError(f"nbr_host must be int32 (n, m), got {nb.shape}")
    n, m = nb.shape
    level, rows = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    level_off = np.empty(n + 1, dtype=np.int32)
    depth = ctypes.c_int64(0)
    as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _check(load().nngp_factor_levels(as_p(nb), n, m, int(trans), as_p(level), as_p(rows), as_p(level_off),
                                     ctypes.byref(depth)), "nngp_factor_levels")
    level_off = np.ascontiguousarray(level_off[:depth.value + 1])
    if device is None:
        return level, rows, level_off
    return FactorSchedule(level, rows, level_off, device)


def _factor_cols(t, name, n):
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 2 or t.shape[0] != n
            or not 1 <= t.shape[1] <= LATENT_MAX_RHS or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float64 ({n}, nrhs) tensor with 1 <= nrhs <= {LATENT_MAX_RHS}")
    return t.shape[1]


def _factor_geom(nbr, B, F=None):
    if nbr.dtype != torch.int32 or nbr.dim() != 2 or not nbr.is_contiguous():
        raise ValueError(f"nbr must be contiguous int32 (n, m), got {nbr.dtype} {tuple(nbr.shape)}")
    n, m = nbr.shape
    if B.dtype != torch.float64 or tuple(B.shape) != (n, m) or not B.is_contiguous():
        raise ValueError(f"B must be contiguous float64 ({n}, {m}), got {B.dtype} {tuple(B.shape)}")
    if F is not None and (F.dtype != torch.float64 or tuple(F.shape) != (n,) or not F.is_contiguous()):
        raise ValueError(f"F must be contiguous float64 ({n},), got {F.dtype} {tuple(F.shape)}")
    return n, m


def _factor_sched(s, n, dev):
    if not isinstance(s, FactorSchedule) or s.rows.shape[0] != n or s.rows_dev.device != dev:
        raise ValueError(f"a FactorSchedule of {n} rows on {dev} is needed (factor_levels(..., device=))")
    return s._args()


def factor_solve_batch(nbr: torch.Tensor, B: torch.Tensor, off, rev_j, rev_k, prep, sched: FactorSchedule,
                       b: torch.Tensor, trans: bool = False, fuse_width: int = 0,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x = (I - B)^-1 b (``trans`` False) or (I - B)^-T b for ``b`` (n, nrhs) (nngp_factor_solve_batch).  ``sched``:
    :func:`factor_levels` of the same ``trans``.  ``out`` may be ``b``.  The transposed solve reads the reverse
    lists and ``prep`` (:func:`reverse_neighbors`, :func:`gibbs_prepare`); the forward solve takes None for them."""
    n, m = _factor_geom(nbr, B)
    nrhs = _factor_cols(b, "b", n)
    dev = _require_gpu(nbr, B, b, out, off, rev_j, rev_k, prep)
    if trans and (off is None or rev_j is None or prep is None):
        raise ValueError("the transposed solve needs off, rev_j and prep")
    if out is None:
        out = torch.empty_like(b)
    elif _factor_cols(out, "out", n) != nrhs:
        raise ValueError("out must have b's shape")
    _check(load().nngp_factor_solve_batch(_ptr(nbr), _ptr(B), _ptr(off), _ptr(rev_j), _ptr(rev_k), _ptr(prep),
                                          *_factor_sched(sched, n, dev), n, m, nrhs, int(bool(trans)),
                                          int(fuse_width), _ptr(b), _ptr(out), _stream(dev)),
           "nngp_factor_solve_batch")
    return out


def factor_cov_apply_batch(nbr: torch.Tensor, B: torch.Tensor, F: torch.Tensor, off, rev_j, rev_k, prep,
                           sched_f: FactorSchedule, sched_t: FactorSchedule, sigma2: float, v: torch.Tensor,
                           fuse_width: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = sigma2 (I - B)^-1 F (I - B)^-T v for ``v`` (n, nrhs) (nngp_factor_cov_apply_batch): the covariance of the
    NNGP prior whose precision :func:`precision_apply_batch` applies with ``d`` None."""
    n, m = _factor_geom(nbr, B, F)
    nrhs = _factor_cols(v, "v", n)
    dev = _require_gpu(nbr, B, F, off, rev_j, rev_k, prep, v, out)
    if out is None:
        out = torch.empty_like(v)
    elif _factor_cols(out, "out", n) != nrhs:
        raise ValueError("out must have v's shape")
    _check(load().nngp_factor_cov_apply_batch(_ptr(nbr), _ptr(B), _ptr(F), _ptr(off), _ptr(rev_j), _ptr(rev_k),
                                              _ptr(prep), *_factor_sched(sched_f, n, dev),
                                              *_factor_sched(sched_t, n, dev), n, m, float(sigma2), nrhs,
                                              int(fuse_width), _ptr(v), _ptr(out), _stream(dev)),
           "nngp_factor_cov_apply_batch")
    return out


def factor_prior_draw_batch(nbr: torch.Tensor, B: torch.Tensor, F: torch.Tensor, sched_f: FactorSchedule,
                            sigma2: float, nrhs: int, fuse_width: int = 0, z: Optional[torch.Tensor] = None,
                            seed: int = 0, draw0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n, nrhs) draws w = (I - B)^-1 (sigma2 F)^1/2 z from the NNGP prior (nngp_factor_prior_draw_batch); ``z``
    (n, nrhs) standard normals, or None: column c is :func:`gibbs_normals` of (seed, sweep = draw0 + c)."""
    n, m = _factor_geom(nbr, B, F)
    nrhs = int(nrhs)
    if not 1 <= nrhs <= LATENT_MAX_RHS:
        raise ValueError(f"nrhs={nrhs} outside [1, {LATENT_MAX_RHS}]")
    if z is not None and _factor_cols(z, "z", n) != nrhs:
        raise ValueError(f"z must have {nrhs} columns")
    dev = _require_gpu(nbr, B, F, z, out)
    if out is None:
        out = torch.empty((n, nrhs), dtype=torch.float64, device=dev)
    elif _factor_cols(out, "out", n) != nrhs:
        raise ValueError(f"out must be ({n}, {nrhs})")
    _check(load().nngp_factor_prior_draw_batch(_ptr(nbr), _ptr(B), _ptr(F), *_factor_sched(sched_f, n, dev), n, m,
                                               float(sigma2), nrhs, int(fuse_width), _ptr(z),
                                               int(seed) & (2 ** 64 - 1), int(draw0), _ptr(out), _stream(dev)),
           "nngp_factor_prior_draw_batch")
    return out
