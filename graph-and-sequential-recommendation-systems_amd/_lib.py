"""ctypes binding of liblgcn_hip.so (include/lgcn_hip.h).

There is NO fallback: if the library cannot be loaded the import of any compute
entry point raises, loudly.  The CPU oracle under oracle/ is test infrastructure
and is never reached from here."""
import ctypes as C
import os

from . import build as _build

F32, BF16, FP8 = 0, 1, 2
ABI_VERSION = 13
MAX_LAYERS = 8
MAX_NEG_RATIO = 16     # LGCN_MAX_NEG_RATIO: negatives per positive of lgcn_train_step_multi / _epoch_multi

LOSS_BPR, LOSS_SOFTMAX, LOSS_INBATCH = 0, 1, 2     # LGCN_LOSS_*: lgcn_ctx_set_loss
LOSS_DIRECTAU = 4                                  # LGCN_LOSS_DIRECTAU: lgcn_ctx_set_directau
SCORE_DOT, SCORE_COSINE = 0, 1                     # LGCN_SCORE_*: lgcn_ctx_set_inbatch_scores
DP_ROWS, DP_DENSE, DP_ROW_SHARDED, DP_COLS = 0, 1, 2, 3                 # LGCN_DP_*: the `reduce` of lgcn_train_epoch_dp
RS_FWD, RS_BPR, RS_SCATTER, RS_BWD, RS_FINISH = 0, 1, 2, 3, 4           # LGCN_RS_*: the phases of lgcn_rs_phase / lgcn_rs_buffer

_c_i32p =C.POINTER(C.c_int32)
_c_i64p = C.POINTER(C.c_int64)
_c_f32p = C.POINTER(C.c_float)
_vp = C.c_void_p


def fp8_col_of_byte(d):
    """Column held by byte b of an fp8 table row (include/lgcn_hip.h, LGCN_FP8): with L = d/16 lanes per row, the 16 bytes at l*16
    hold the four 4-column chunks j*L + l, j = 0..3  ->  int64 [d]."""
    import numpy as np
    b = np.arange(d)
    l, j, e = b // 16, (b % 16) // 4, b % 4
    return ((j * (d // 16) + l) * 4 + e).astype(np.int64)


class TrainConfig(C.Structure):
    """Mirror of lgcn_train_config (include/lgcn_hip.h)."""
    _fields_ = [
        ("graph", _vp),
        ("n_users", C.c_int32), ("d", C.c_int32), ("K", C.c_int32), ("act_dtype", C.c_int32),
        ("E0", _vp), ("adam_m", _vp), ("adam_v", _vp),
        ("act", _vp), ("G64", _vp), ("bitmap", _vp), ("terms", _vp), ("contrib", _vp),
        ("err", _vp), ("max_batch", C.c_int32),
        ("decay", C.c_float),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
        ("xcd_remap", C.c_int32), ("dense_last", C.c_int32),
        ("hub_nnz", C.c_int32), ("hub_chunk", C.c_int32),
        ("i2i", _vp), ("i2i_t", _vp),
        ("item_pop", _vp), ("gate_params", _vp), ("gate_adam_m", _vp), ("gate_adam_v", _vp), ("gate_grad", _vp),
        ("pop_hidden", C.c_int32), ("gate_hidden", C.c_int32),
        ("gate_entropy_coeff", C.c_float), ("pop_gate_temp", C.c_float),
        ("reg_ego", C.c_int32),
    ]


class MfConfig(C.Structure):
    """Mirror of lgcn_mf_config (include/lgcn_hip.h)."""
    _fields_ = [
        ("n_users", C.c_int32), ("m_items", C.c_int32), ("d", C.c_int32),
        ("E0", _vp), ("adam_m", _vp), ("adam_v", _vp),
        ("G64", _vp), ("bitmap", _vp), ("terms", _vp),
        ("err", _vp), ("max_batch", C.c_int32),
        ("decay", C.c_float),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
    ]


# name -> (restype, argtypes); every symbol include/lgcn_hip.h declares
SIGNATURES = {
    "lgcn_abi_version": (C.c_int, []),
    "lgcn_last_error": (C.c_char_p, []),
    "lgcn_device_available": (C.c_int, []),
    "lgcn_np_shuffle_perm_device_workspace": (C.c_int64, [C.c_int64]),
    "lgcn_np_shuffle_perm_device": (C.c_int, [C.c_int64, _vp, _vp, C.c_int64, _vp]),
    "lgcn_table_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "lgcn_to_fp8": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp]),
    "lgcn_sampling_seed": (None, [C.c_uint]),
    "lgcn_sampling_randint": (C.c_int, [C.c_int]),
    "lgcn_sample_negative": (C.c_int, [C.c_int, C.c_int, C.c_int64, _vp, _vp, C.c_int, _vp]),
    "lgcn_sample_negative_by_user": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp]),
    "lgcn_sample_negative_device_workspace": (C.c_int64, [C.c_int, C.c_int64]),
    "lgcn_sampler_test_margin": (None, [C.c_int64, C.c_int64]),
    "lgcn_sample_negative_device": (C.c_int, [C.c_int, C.c_int, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "lgcn_sample_negative_device_multi_workspace": (C.c_int64, [C.c_int, C.c_int64, C.c_int]),
    "lgcn_sample_negative_device_multi": (C.c_int, [C.c_int, C.c_int, C.c_int64, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int64, _vp]),
    "lgcn_np_seed": (None, [C.c_uint32]),
    "lgcn_np_get_state": (None, [_vp, C.POINTER(C.c_uint32)]),
    "lgcn_np_set_state": (None, [_vp, C.c_uint32]),
    "lgcn_fy_resolve_device": (C.c_int, [_vp, C.c_int64, _vp, _vp, C.c_int64, _vp]),     # test hook
    "lgcn_sample_python": (C.c_int64, [C.c_int, C.c_int, C.c_int64, _vp, _vp, _vp]),
    "lgcn_np_shuffle_perm": (C.c_int, [C.c_int64, _vp]),
    "lgcn_build_user_item_csr": (C.c_int, [C.c_int, C.c_int, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lgcn_adj_rowsum": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "lgcn_build_norm_adj": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lgcn_graph_create": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int32, _vp, C.c_int64, _vp, C.POINTER(_vp)]),
    "lgcn_graph_destroy": (None, [_vp]),
    "lgcn_spmm_csr": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp]),
    "lgcn_propagate_mean": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "lgcn_apply_perm": (C.c_int, [_vp, C.c_int, _vp, C.c_int64, _vp, _vp, _vp, _vp]),
    "lgcn_ctx_create": (C.c_int, [C.POINTER(TrainConfig), C.POINTER(_vp)]),
    "lgcn_ctx_destroy": (None, [_vp]),
    "lgcn_ctx_get_step": (C.c_int64, [_vp]),
    "lgcn_ctx_hub_rows": (C.c_int64, [_vp]),
    "lgcn_ctx_set_step": (None, [_vp, C.c_int64]),
    "lgcn_ctx_set_lr": (None, [_vp, C.c_double]),
    "lgcn_ctx_set_dp_local": (C.c_int, [_vp, C.c_int]),
    "lgcn_train_step": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "lgcn_train_epoch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, _vp, _vp]),
    # several negatives per positive (--neg_ratio)
    "lgcn_apply_perm_multi": (C.c_int, [_vp, C.c_int, _vp, C.c_int64, _vp, _vp, _vp, C.c_int32, _vp]),
    "lgcn_train_step_multi": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp]),
    "lgcn_train_epoch_multi": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int64, C.c_int32, _vp, _vp]),
    # the loss of the multi-negative step (--loss)
    "lgcn_ctx_set_loss": (C.c_int, [_vp, C.c_int32, C.c_float]),
    "lgcn_ctx_get_loss": (C.c_int32, [_vp, _vp]),
    # the in-batch sampled softmax (--loss inbatch)
    "lgcn_train_step_inbatch": (C.c_int, [_vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "lgcn_train_epoch_inbatch": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int32, _vp, _vp]),
    # its score options (--score, --inbatch_logq)
    "lgcn_ctx_set_inbatch_scores": (C.c_int, [_vp, C.c_int, _vp]),
    "lgcn_ctx_get_inbatch_scores": (C.c_int, [_vp, C.POINTER(_vp)]),
    # mixed negatives for the in-batch step (--inbatch_mix)
    "lgcn_ctx_set_inbatch_mix": (C.c_int, [_vp, C.c_int32]),
    "lgcn_ctx_get_inbatch_mix": (C.c_int32, [_vp]),
    "lgcn_train_step_inbatch_mix": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp]),
    "lgcn_train_epoch_inbatch_mix": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int64, C.c_int32, _vp, _vp]),
    # the alignment-and-uniformity loss (--loss directau, --au_gamma)
    "lgcn_ctx_set_directau": (C.c_int, [_vp, C.c_float]),
    "lgcn_ctx_get_directau": (C.c_int, [_vp, _vp]),
    "lgcn_train_step_directau": (C.c_int, [_vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "lgcn_train_epoch_directau": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int32, _vp, _vp]),
    # hard negatives for the multi-negative step, DNS(M, N) (--hard_neg)
    "lgcn_ctx_set_hard_neg": (C.c_int, [_vp, C.c_int32, C.c_uint64, _vp]),
    "lgcn_ctx_get_hard_neg": (C.c_int32, [_vp]),
    "lgcn_hard_neg_rank": (C.c_uint32, [C.c_uint64, C.c_int64, C.c_int32, C.c_int32]),
    "lgcn_dp_block_floats": (C.c_int64, [_vp, C.c_int32, C.c_int32]),
    "lgcn_train_step_dp_part1": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp]),
    "lgcn_train_step_dp_dense_part1": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp]),
    "lgcn_ctx_gate_total": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "lgcn_train_step_dp_part2": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "lgcn_ctx_check": (C.c_int, [_vp, _vp]),
    "lgcn_eval_topk": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "lgcn_eval_topk_masked": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp]),
    "lgcn_eval_mask_words": (C.c_int64, [C.c_int32, C.c_int32]),
    "lgcn_eval_build_masks": (C.c_int, [_vp, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp]),
    "lgcn_eval_topk_fp32": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "lgcn_eval_metrics": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "lgcn_eval_kmax": (C.c_int32, []),
    "lgcn_eval_topk_ex": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp, _vp,
                                    C.c_int64, C.c_int32, _vp]),
    "lgcn_eval_metrics_ex": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "lgcn_eval_ranks": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp,
                                  C.c_int32, _vp]),
    "lgcn_eval_rank_metrics": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_int32,
                                         _vp, _vp, _vp]),
    "lgcn_eval_pop_metrics": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_int32, _vp, C.c_int32,
                                        _vp, _vp, _vp, _vp, _vp, _vp]),
    "lgcn_i2i_topk": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "lgcn_i2i_finish": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp, C.POINTER(C.c_int64), _vp]),
    "lgcn_dp_available": (C.c_int, []),
    "lgcn_dp_unique_id": (C.c_int, [_vp]),
    "lgcn_dp_init": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "lgcn_train_step_i64": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "lgcn_train_step_cols_part1": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.POINTER(_vp), _vp]),
    "lgcn_train_step_cols_part2": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "lgcn_dp_allreduce_sum_f32": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "lgcn_dp_init_loopback": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "lgcn_dp_destroy": (None, [_vp]),
    "lgcn_dp_world": (C.c_int, [_vp]),
    "lgcn_dp_rank": (C.c_int, [_vp]),
    "lgcn_train_epoch_dp": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "lgcn_rs_phase": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "lgcn_rs_buffer": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(_vp), C.POINTER(C.c_int32)]),
    "lgcn_ctx_set_dropout": (C.c_int, [_vp, C.c_float, C.c_uint64]),
    "lgcn_ctx_set_layer_weights": (C.c_int, [_vp, _vp, C.c_int32]),
    "lgcn_ctx_get_layer_weights": (C.c_int32, [_vp, _vp]),
    "lgcn_propagate_weighted": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "lgcn_dropout_mask": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_float, C.c_uint64, C.c_int64, _vp, _vp]),
    "lgcn_spmm_csr_drop": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int64, C.c_int, _vp]),
    "lgcn_mf_create": (C.c_int, [C.POINTER(MfConfig), C.POINTER(_vp)]),
    "lgcn_mf_destroy": (None, [_vp]),
    "lgcn_mf_get_step": (C.c_int64, [_vp]),
    "lgcn_mf_set_step": (None, [_vp, C.c_int64]),
    "lgcn_mf_set_lr": (None, [_vp, C.c_double]),
    "lgcn_mf_train_step": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "lgcn_mf_train_epoch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, _vp, _vp]),
    "lgcn_mf_check": (C.c_int, [_vp, _vp]),
    "lgcn_ctx_set_fold_g32": (C.c_int, [_vp, C.c_int]),
    "lgcn_ctx_folded_steps": (C.c_int64, [_vp]),
    "lgcn_ctx_copy_arrivals": (C.c_int, [_vp, _vp, C.c_int64]),
    "lgcn_slot_multiplicity": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int64, _vp, _vp]),
    # write-through stores for outputs nobody gathers
    "lgcn_ctx_set_store_policy": (C.c_int, [_vp, C.c_int]),
    "lgcn_ctx_get_store_policy": (C.c_int, [_vp, _c_i32p]),
}

STORE_ADAM, STORE_XLAST = 1, 2                       # LGCN_STORE_*: lgcn_ctx_set_store_policy
STORE_ARG_MV, STORE_ARG_P, STORE_ARG_Y = 1, 2, 4     # LGCN_STORE_ARG_*: what a launch carried (lgcn_ctx_get_store_policy)

_LIB = None


class LgcnError(RuntimeError):
    pass


def load():
    """Load liblgcn_hip.so.  A stale or missing library is rebuilt first -- except inside a rank of
    a distributed job or under a profiler, where the library must already exist (build it once
    with `python -m graph-and-sequential-recommendation-systems_amd.build` or __graft_entry__.build()).
    Raises if impossible."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB_PATH
    if os.environ.get("LGCN_LIB_PATH"):
        pass                                   # explicit tuning variant: use as is
    elif _build.is_stale():
        if _build.must_not_build():
            if not os.path.exists(path):
                raise LgcnError(
                    f"liblgcn_hip.so is missing at {path}; this process is a distributed rank or runs under a "
                    "profiler and will not compile it. Build it first (__graft_entry__.build()).")
            # present but not provably current (e.g. built by hand with other flags): use it
        elif _build.find_hipcc() is not None:
            _build.build()
        elif not os.path.exists(path):
            raise LgcnError(
                f"liblgcn_hip.so is missing at {path} and hipcc is not available to build it. "
                "The MI355X HIP library is the product path; there is no CPU fallback.")
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise LgcnError(f"cannot load {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise LgcnError(f"{path} does not export {name} (stale build?)") from e
        fn.restype, fn.argtypes = res, args
    if lib.lgcn_abi_version() != ABI_VERSION:
        raise LgcnError("liblgcn_hip.so ABI version mismatch")
    _LIB = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().lgcn_last_error()
        raise LgcnError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def npp(a):
    """numpy array -> void* (array must stay alive for the call)."""
    return a.ctypes.data_as(_vp)


def tp(t):
    """torch tensor -> void* device/host pointer."""
    return _vp(t.data_ptr()) if t is not None else _vp(0)


def require_gpu():
    import torch
    if not torch.cuda.is_available() or not load().lgcn_device_available():
        raise LgcnError("no MI355X/HIP device visible: the LightGCN HIP kernels cannot run "
                        "(there is deliberately no CPU fallback)")


def current_stream():
    import torch
    return _vp(torch.cuda.current_stream().cuda_stream)


EVAL_FP32 = 1          # LGCN_EVAL_FP32


def eval_kmax():
    """Largest K of the fused evaluation (lgcn_eval_kmax)."""
    return int(load().lgcn_eval_kmax())


def _want(t, name, dtype, shape, dev=None):
    """ValueError unless t is a contiguous tensor of this dtype and shape (on dev when given)."""
    import torch
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} must be on {dev}, got {t.device}")


def eval_topk(E, n_users, users32, train_ptr, train_idx32, K, out_items, out_scores=None, masks=None, fp32=False):
    """lgcn_eval_topk_ex, checked: E the propagated table [n_users + m_items, d] fp32 on the device, users32 int32 [n_eval],
    train_ptr int64 [n_users + 1], train_idx32 int32, out_items int32 [n_eval, K] (out_scores fp32 [n_eval, K] or None),
    masks from lgcn_eval_build_masks or None.  Everything is validated before anything is launched (ValueError)."""
    import torch
    _want(E, "E", torch.float32, None)
    if E.dim() != 2 or E.device.type != "cuda":
        raise ValueError("E must be a 2-D device tensor")
    dev = E.device
    n_users, d = int(n_users), int(E.shape[1])
    m_items = int(E.shape[0]) - n_users
    if d not in (32, 64, 128, 256) or n_users <= 0 or m_items <= 0:
        raise ValueError(f"E [{tuple(E.shape)}] with n_users={n_users}: d must be 32, 64, 128 or 256 and both sides non-empty")
    K = int(K)
    if not 1 <= K <= eval_kmax() or K > m_items:
        raise ValueError(f"K={K} must be in 1..{eval_kmax()} and <= m_items={m_items}")
    _want(users32, "users32", torch.int32, None, dev)
    n = int(users32.numel())
    _want(train_ptr, "train_ptr", torch.int64, None, dev)
    if train_ptr.dim() != 1 or train_ptr.numel() < n_users + 1:
        raise ValueError(f"train_ptr must hold n_users + 1 = {n_users + 1} offsets")
    _want(train_idx32, "train_idx32", torch.int32, None, dev)
    _want(out_items, "out_items", torch.int32, (n, K), dev)
    if out_scores is not None:
        _want(out_scores, "out_scores", torch.float32, (n, K), dev)
    if masks is not None:
        _want(masks, "masks", torch.int32, (int(load().lgcn_eval_mask_words(m_items, n)),), dev)
    check(load().lgcn_eval_topk_ex(tp(E), n_users, m_items, d, tp(users32), n, tp(train_ptr), tp(train_idx32), tp(masks),
                                   K, tp(out_items), tp(out_scores), n * K, EVAL_FP32 if fp32 else 0, current_stream()),
          "lgcn_eval_topk_ex")
    return out_items


def eval_metrics(topk, test_ptr, test_sorted32, ks, per_user=None, sums=None):
    """lgcn_eval_metrics_ex, checked: topk int32 [n_eval, K] on the device, test_ptr int64 [n_eval + 1], test_sorted32 int32 (ids
    ascending per slot), ks 1..8 cut-offs in 1..K.  Returns (per_user float64 [n_eval, 3 len(ks)], sums float64 [3 len(ks)])."""
    import torch
    if not torch.is_tensor(topk) or topk.dim() != 2:
        raise ValueError("topk must be a 2-D tensor")
    dev = topk.device
    _want(topk, "topk", torch.int32, None)
    if dev.type != "cuda":
        raise ValueError("topk must be a device tensor")
    n, K = int(topk.shape[0]), int(topk.shape[1])
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= 8 or any(not 1 <= k <= K for k in ks) or not 1 <= K <= eval_kmax():
        raise ValueError(f"1..8 cut-offs in 1..K (K={K} <= {eval_kmax()}), got {ks}")
    _want(test_ptr, "test_ptr", torch.int64, (n + 1,), dev)
    _want(test_sorted32, "test_sorted32", torch.int32, None, dev)
    if per_user is None:
        per_user = torch.empty(n, 3 * len(ks), dtype=torch.float64, device=dev)
    if sums is None:
        sums = torch.empty(3 * len(ks), dtype=torch.float64, device=dev)
    _want(per_user, "per_user", torch.float64, (n, 3 * len(ks)), dev)
    _want(sums, "sums", torch.float64, (3 * len(ks),), dev)
    ks_h = torch.tensor(ks, dtype=torch.int32)
    check(load().lgcn_eval_metrics_ex(tp(topk), n, K, tp(test_ptr), tp(test_sorted32), tp(ks_h), len(ks), tp(per_user), tp(sums),
                                      current_stream()), "lgcn_eval_metrics_ex")
    return per_user, sums


def _rank_lists(users32, train_ptr, train_idx32, test_ptr, test_sorted32, n_users=None):
    """Shared checks of the rank entry points: returns (dev, n_eval, n_test)."""
    import torch
    _want(users32, "users32", torch.int32, None)
    if users32.dim() != 1 or users32.device.type != "cuda":
        raise ValueError("users32 must be a 1-D device tensor")
    dev = users32.device
    n = int(users32.numel())
    _want(train_ptr, "train_ptr", torch.int64, None, dev)
    if train_ptr.dim() != 1 or train_ptr.numel() < 2 or (n_users is not None and train_ptr.numel() < n_users + 1):
        raise ValueError("train_ptr must hold n_users + 1 offsets")
    _want(train_idx32, "train_idx32", torch.int32, None, dev)
    _want(test_ptr, "test_ptr", torch.int64, (n + 1,), dev)
    _want(test_sorted32, "test_sorted32", torch.int32, None, dev)
    if test_sorted32.dim() != 1:
        raise ValueError("test_sorted32 must be 1-D")
    return dev, n, int(test_sorted32.numel())


def eval_ranks(E, n_users, users32, train_ptr, train_idx32, test_ptr, test_sorted32, scores=None, gt=None, eq=None, fp32=False):
    """lgcn_eval_ranks, checked: E the propagated table [n_users + m_items, d] fp32 on the device, users32 int32 [n_eval],
    the train CSR (int64 train_ptr [n_users + 1], int32 ids ascending), the test CSR over the slots (int64 test_ptr
    [n_eval + 1], test_sorted32 int32 [n_test], ids ascending per slot; test_ptr[n_eval] must be n_test -- the caller's
    contract, not read back here).  Returns (scores fp32, gt int32, eq int32), each [n_test]; buffers passed in must have
    exactly that shape.  Everything is validated before anything is launched (ValueError)."""
    import torch
    _want(E, "E", torch.float32, None)
    if E.dim() != 2 or E.device.type != "cuda":
        raise ValueError("E must be a 2-D device tensor")
    n_users, d = int(n_users), int(E.shape[1])
    m_items = int(E.shape[0]) - n_users
    if d not in (32, 64, 128, 256) or n_users <= 0 or m_items <= 0:
        raise ValueError(f"E [{tuple(E.shape)}] with n_users={n_users}: d must be 32, 64, 128 or 256 and both sides non-empty")
    dev, n, n_test = _rank_lists(users32, train_ptr, train_idx32, test_ptr, test_sorted32, n_users)
    if dev != E.device:
        raise ValueError(f"users32 must be on {E.device}")
    if n_test > n * m_items:
        raise ValueError(f"n_test={n_test} exceeds n_eval * m_items")
    if scores is None:
        scores = torch.empty(n_test, dtype=torch.float32, device=dev)
    if gt is None:
        gt = torch.empty(n_test, dtype=torch.int32, device=dev)
    if eq is None:
        eq = torch.empty(n_test, dtype=torch.int32, device=dev)
    _want(scores, "scores", torch.float32, (n_test,), dev)
    _want(gt, "gt", torch.int32, (n_test,), dev)
    _want(eq, "eq", torch.int32, (n_test,), dev)
    check(load().lgcn_eval_ranks(tp(E), n_users, m_items, d, tp(users32), n, tp(train_ptr), tp(train_idx32), tp(test_ptr),
                                 tp(test_sorted32), n_test, tp(scores), tp(gt), tp(eq), EVAL_FP32 if fp32 else 0,
                                 current_stream()), "lgcn_eval_ranks")
    return scores, gt, eq


def eval_rank_metrics(m_items, users32, train_ptr, train_idx32, test_ptr, test_sorted32, scores, gt, eq, ks, per_user=None, sums=None):
    """lgcn_eval_rank_metrics, checked: the lists as eval_ranks, its three outputs, ks 1..8 cut-offs in 1..m_items.  Returns
    (per_user float64 [n_eval, 3 len(ks) + 2] = precision | recall | ndcg | auc | mrr, sums float64 [3 len(ks) + 2])."""
    import torch
    m_items = int(m_items)
    ks = [int(k) for k in ks]
    if m_items <= 0 or not 1 <= len(ks) <= 8 or any(not 1 <= k <= m_items for k in ks):
        raise ValueError(f"1..8 cut-offs in 1..m_items={m_items}, got {ks}")
    dev, n, n_test = _rank_lists(users32, train_ptr, train_idx32, test_ptr, test_sorted32)
    _want(scores, "scores", torch.float32, (n_test,), dev)
    _want(gt, "gt", torch.int32, (n_test,), dev)
    _want(eq, "eq", torch.int32, (n_test,), dev)
    width = 3 * len(ks) + 2
    if per_user is None:
        per_user = torch.empty(n, width, dtype=torch.float64, device=dev)
    if sums is None:
        sums = torch.empty(width, dtype=torch.float64, device=dev)
    _want(per_user, "per_user", torch.float64, (n, width), dev)
    _want(sums, "sums", torch.float64, (width,), dev)
    ks_h = torch.tensor(ks, dtype=torch.int32)
    check(load().lgcn_eval_rank_metrics(n, m_items, tp(users32), tp(train_ptr), tp(train_idx32), tp(test_ptr), tp(test_sorted32),
                                        n_test, tp(scores), tp(gt), tp(eq), tp(ks_h), len(ks), tp(per_user), tp(sums),
                                        current_stream()), "lgcn_eval_rank_metrics")
    return per_user, sums


def eval_pop_metrics(topk, test_ptr, test_sorted32, item_info, n_groups, ks, exposure=None, per_slot=None, want_exposure=False):
    """lgcn_eval_pop_metrics, checked: topk int32 [n_eval, K] on the device, the test CSR as eval_metrics takes it, item_info
    int32 [m_items] (utils.pack_item_info: pop * 8 + group), 1 <= n_groups <= 8, ks 1..8 cut-offs in 1..K.  Returns a dict of
    device tensors: sums float64 [n_ks, 2, n_groups], counts int64 [n_ks, n_groups + 5], group_slots int64 [n_groups] (views of
    'packed', one int64 buffer: pop_unpack reads its host copy), and
    exposure int32 [n_ks, m_items] / per_slot float64 [n_eval, n_ks, 2, n_groups] or None (exposure is allocated with
    want_exposure).  Everything is validated before any pointer leaves Python (ValueError)."""
    import torch
    if not torch.is_tensor(topk) or topk.dim() != 2:
        raise ValueError("topk must be a 2-D tensor")
    dev = topk.device
    _want(topk, "topk", torch.int32, None)
    if dev.type != "cuda":
        raise ValueError("topk must be a device tensor")
    n, K = int(topk.shape[0]), int(topk.shape[1])
    ks = [int(k) for k in ks]
    G = int(n_groups)
    if not 1 <= G <= 8:
        raise ValueError(f"n_groups must be in 1..8, got {n_groups}")
    if not 1 <= len(ks) <= 8 or any(not 1 <= k <= K for k in ks) or not 1 <= K <= eval_kmax():
        raise ValueError(f"1..8 cut-offs in 1..K (K={K} <= {eval_kmax()}), got {ks}")
    _want(test_ptr, "test_ptr", torch.int64, (n + 1,), dev)
    _want(test_sorted32, "test_sorted32", torch.int32, None, dev)
    if test_sorted32.dim() != 1:
        raise ValueError("test_sorted32 must be 1-D")
    _want(item_info, "item_info", torch.int32, None, dev)
    if item_info.dim() != 1 or item_info.numel() < 1:
        raise ValueError("item_info must be 1-D with one word per item")
    m_items = int(item_info.numel())
    if n * K * m_items >= 1 << 62:
        raise ValueError(f"n_eval * K * m_items = {n * K * m_items} reaches 2^62: the Gini numerator could leave int64")
    nk = len(ks)
    if exposure is None and want_exposure:
        exposure = torch.empty(nk, m_items, dtype=torch.int32, device=dev)
    if exposure is not None:
        _want(exposure, "exposure", torch.int32, (nk, m_items), dev)
    if per_slot is not None:
        _want(per_slot, "per_slot", torch.float64, (n, nk, 2, G), dev)
    packed = torch.empty(nk * 2 * G + nk * (G + 5) + G, dtype=torch.int64, device=dev)     # one buffer: one copy brings all sums to the host
    sums, counts, group_slots = pop_unpack(packed, nk, G)
    ks_h = torch.tensor(ks, dtype=torch.int32)
    check(load().lgcn_eval_pop_metrics(tp(topk), n, K, tp(test_ptr), tp(test_sorted32), tp(item_info), m_items, G, tp(ks_h), nk,
                                       tp(sums), tp(counts), tp(group_slots), tp(exposure), tp(per_slot), current_stream()),
          "lgcn_eval_pop_metrics")
    return {'sums': sums, 'counts': counts, 'group_slots': group_slots, 'exposure': exposure, 'per_slot': per_slot, 'packed': packed}


def pop_unpack(packed, nk, G):
    """(sums float64 [nk, 2, G], counts int64 [nk, G + 5], group_slots int64 [G]) as views of eval_pop_metrics' one int64 buffer
    (a torch tensor, or its host copy as a numpy array)."""
    import numpy as np
    import torch
    a, b = nk * 2 * G, nk * 2 * G + nk * (G + 5)
    sums = packed[:a].view(np.float64 if isinstance(packed, np.ndarray) else torch.float64)
    return sums.reshape(nk, 2, G), packed[a:b].reshape(nk, G + 5), packed[b:]


I2I_WEIGHTS = {"cooc": 0, "jaccard": 1, "pmi": 2}       # LGCN_I2I_COOC / _JACCARD / _PMI
I2I_TOPK_MAX = 256


def _i2i_sizes(m_items, topk):
    m_items, topk = int(m_items), int(topk)
    if m_items <= 0:
        raise ValueError(f"m_items={m_items} must be positive")
    if not 1 <= topk <= I2I_TOPK_MAX:
        raise ValueError(f"topk={topk} must be in 1..{I2I_TOPK_MAX}")
    if 2 * m_items * topk >= 2 ** 31 - 16:
        raise ValueError(f"2 * m_items * topk = {2 * m_items * topk} must stay below 2^31")
    return m_items, topk


def i2i_topk(indptr, indices, m_items, topk=50, weight="cooc", min_basket=1, cols=None, w=None, length=None):
    """lgcn_i2i_topk, checked: baskets as a device CSR (indptr int64 [n_baskets + 1], indices int32 [nnz], items distinct within
    a basket) -> (cols int32 [m_items, topk] in rank order padded with -1, w fp32 [m_items, topk], len int32 [m_items]).
    Everything the host can see is validated before anything is launched (ValueError); an id outside [0, m_items) is found on
    the device (LgcnError, outputs untouched)."""
    import torch
    m_items, topk = _i2i_sizes(m_items, topk)
    if weight not in I2I_WEIGHTS:
        raise ValueError(f"weight must be one of {sorted(I2I_WEIGHTS)}, got {weight!r}")
    min_basket = int(min_basket)
    if min_basket < 0:
        raise ValueError(f"min_basket={min_basket} must be >= 0")
    _want(indptr, "indptr", torch.int64, None)
    if indptr.dim() != 1 or indptr.numel() < 2 or indptr.device.type != "cuda":
        raise ValueError("indptr must be a 1-D device tensor of n_baskets + 1 >= 2 offsets")
    dev = indptr.device
    _want(indices, "indices", torch.int32, None, dev)
    if indices.dim() != 1 or indices.numel() == 0:
        raise ValueError("indices must be a non-empty 1-D tensor")
    n_baskets, nnz = int(indptr.numel()) - 1, int(indices.numel())
    if cols is None:
        cols = torch.empty(m_items, topk, dtype=torch.int32, device=dev)
    if w is None:
        w = torch.empty(m_items, topk, dtype=torch.float32, device=dev)
    if length is None:
        length = torch.empty(m_items, dtype=torch.int32, device=dev)
    _want(cols, "cols", torch.int32, (m_items, topk), dev)
    _want(w, "w", torch.float32, (m_items, topk), dev)
    _want(length, "length", torch.int32, (m_items,), dev)
    check(load().lgcn_i2i_topk(tp(indptr), tp(indices), n_baskets, nnz, m_items, topk, I2I_WEIGHTS[weight], min_basket,
                               tp(cols), tp(w), tp(length), current_stream()), "lgcn_i2i_topk")
    return cols, w, length


def i2i_finish(cols, w, length, capacity=None, indptr=None, indices=None, vals=None):
    """lgcn_i2i_finish, checked: the three arrays of i2i_topk -> (indptr int32 [m_items + 1], indices int32 [capacity],
    vals fp32 [capacity], nnz): symmetrised by maximum, D^-1/2 A D^-1/2, columns ascending.  capacity (default
    2 * m_items * topk, always enough) must be at least 2 * sum(len): checked on the device (LgcnError, outputs untouched)."""
    import torch
    if not torch.is_tensor(cols) or cols.dim() != 2 or cols.device.type != "cuda":
        raise ValueError("cols must be a 2-D device tensor [m_items, topk]")
    dev = cols.device
    m_items, topk = _i2i_sizes(cols.shape[0], cols.shape[1])
    _want(cols, "cols", torch.int32, None)
    _want(w, "w", torch.float32, (m_items, topk), dev)
    _want(length, "length", torch.int32, (m_items,), dev)
    capacity = 2 * m_items * topk if capacity is None else int(capacity)
    if capacity <= 0:
        raise ValueError(f"capacity={capacity} must be positive")
    if indptr is None:
        indptr = torch.empty(m_items + 1, dtype=torch.int32, device=dev)
    if indices is None:
        indices = torch.empty(capacity, dtype=torch.int32, device=dev)
    if vals is None:
        vals = torch.empty(capacity, dtype=torch.float32, device=dev)
    _want(indptr, "indptr", torch.int32, (m_items + 1,), dev)
    _want(indices, "indices", torch.int32, (capacity,), dev)
    _want(vals, "vals", torch.float32, (capacity,), dev)
    nnz = C.c_int64(-1)
    check(load().lgcn_i2i_finish(tp(cols), tp(w), tp(length), m_items, topk, capacity, tp(indptr), tp(indices), tp(vals),
                                 C.byref(nnz), current_stream()), "lgcn_i2i_finish")
    return indptr, indices, vals, int(nnz.value)


class Graph:
    """Owner of an lgcn_graph handle over device CSR tensors (kept alive here)."""

    def __init__(self, indptr, indices, vals, d_max=256, row_order=None, xcd_start=None):
        import numpy as np
        import torch
        require_gpu()
        self.indptr = indptr.to(torch.int32).contiguous()
        self.indices = indices.to(torch.int32).contiguous()
        self.vals = vals.to(torch.float32).contiguous()
        if self.indices.numel() == 0:        # keep pointers non-null for an empty matrix
            self.indices = torch.zeros(1, dtype=torch.int32, device=self.indptr.device)
            self.vals = torch.zeros(1, dtype=torch.float32, device=self.indptr.device)
            nnz = 0
        else:
            nnz = int(indices.numel())
        self.n_rows = int(self.indptr.numel()) - 1
        self.nnz = nnz
        self.d_max = int(d_max)
        self.row_order = None
        if row_order is not None:
            self.row_order = torch.as_tensor(row_order).to(device=self.indptr.device, dtype=torch.int32).contiguous()
        xs = None
        if xcd_start is not None:
            xs = np.ascontiguousarray(xcd_start, np.int64)
            if xs.shape != (9,):
                raise LgcnError("Graph: xcd_start must hold 9 positions")
        h = _vp()
        check(load().lgcn_graph_create(tp(self.indptr), tp(self.indices), tp(self.vals), self.n_rows, nnz,
                                       int(d_max), tp(self.row_order),
                                       int(self.row_order.numel()) if self.row_order is not None else self.n_rows,
                                       npp(xs) if xs is not None else None, C.byref(h)), "lgcn_graph_create")
        self.handle = h

    def to_fp8(self, x):
        """fp32 [n_rows, d] -> the library's fp8 table (uint8 tensor: n_rows*d E4M3 bytes, then n_rows fp32 row scales, padded)."""
        import torch
        x = x.contiguous().float()
        n, d = int(x.shape[0]), int(x.shape[1])
        out = torch.zeros(int(load().lgcn_table_bytes(n, d, FP8)), dtype=torch.uint8, device=x.device)
        check(load().lgcn_to_fp8(tp(x), tp(out), n, d, current_stream()), "lgcn_to_fp8")
        return out

    @staticmethod
    def from_fp8(tab, n, d):
        """decode an fp8 table (as to_fp8 / an fp8 SpMM output lays it out) to fp32 [n, d] with torch (test helper)"""
        import torch
        q = tab[:n * d].view(torch.float8_e4m3fn).view(n, d).float()
        sc = tab[n * d:n * d + 4 * n].view(torch.float32)
        out = torch.empty_like(q)
        out[:, torch.from_numpy(fp8_col_of_byte(d)).to(q.device)] = q           # the bytes of a row are chunk-interleaved
        return out * sc[:, None]

    def spmm_fp8(self, xq, d, y_dtype=FP8):
        """A @ X for an fp8 table xq (see to_fp8): -> fp8 table (y_dtype FP8) or fp32 [n_rows, d] (F32)."""
        import torch
        if y_dtype == FP8:
            y = torch.zeros(int(load().lgcn_table_bytes(self.n_rows, d, FP8)), dtype=torch.uint8, device=xq.device)
        else:
            y = torch.empty(self.n_rows, d, dtype=torch.float32, device=xq.device)
        check(load().lgcn_spmm_csr(self.handle, tp(xq), FP8, tp(y), y_dtype, int(d), current_stream()), "lgcn_spmm_csr")
        return y

    def spmm(self, x, y_dtype=None):
        import torch
        if x.dim() != 2 or x.shape[0] != self.n_rows or x.shape[1] not in (32, 64, 128, 256) or x.shape[1] > self.d_max:
            raise LgcnError(f"Graph.spmm: x must be [{self.n_rows}, d] with d in (32,64,128,256) and d <= d_max={self.d_max}; "
                            f"got {tuple(x.shape)}")
        if x.device != self.indptr.device:
            raise LgcnError("Graph.spmm: x is not on the graph's device")
        x = x.contiguous()
        xd = BF16 if x.dtype == torch.bfloat16 else F32
        if xd == F32:
            x = x.float()
        yd = xd if y_dtype is None else y_dtype
        if yd == FP8:
            y = torch.zeros(int(load().lgcn_table_bytes(self.n_rows, int(x.shape[1]), FP8)), dtype=torch.uint8, device=x.device)
        else:
            y = torch.empty(x.shape, dtype=torch.bfloat16 if yd == BF16 else torch.float32, device=x.device)
        check(load().lgcn_spmm_csr(self.handle, tp(x), xd, tp(y), yd, int(x.shape[1]), current_stream()), "lgcn_spmm_csr")
        return y

    def dropout_mask(self, keep_prob, seed, step):
        """lgcn_dropout_mask on this graph's CSR: uint8 [nnz], 1 where the entry at that CSR position is kept in step `step`."""
        import torch
        out = torch.empty(max(self.nnz, 1), dtype=torch.uint8, device=self.indptr.device)
        check(load().lgcn_dropout_mask(tp(self.indptr), tp(self.indices), self.n_rows, self.nnz, float(keep_prob),
                                       int(seed) & (2 ** 64 - 1), int(step), tp(out), current_stream()), "lgcn_dropout_mask")
        return out[:self.nnz]

    def spmm_drop(self, x, keep_prob, seed, step, transposed=False, y_dtype=None):
        """lgcn_spmm_csr_drop: A_drop @ x (or A_drop^T @ x) with the edge-dropout mask of (seed, step); x fp32 or bf16."""
        import torch
        if x.dim() != 2 or x.shape[0] != self.n_rows or x.shape[1] not in (32, 64, 128, 256) or x.shape[1] > self.d_max:
            raise LgcnError(f"Graph.spmm_drop: x must be [{self.n_rows}, d] with d in (32,64,128,256) and d <= d_max={self.d_max}; "
                            f"got {tuple(x.shape)}")
        if x.device != self.indptr.device:
            raise LgcnError("Graph.spmm_drop: x is not on the graph's device")
        x = x.contiguous()
        xd = BF16 if x.dtype == torch.bfloat16 else F32
        if xd == F32:
            x = x.float()
        yd = xd if y_dtype is None else y_dtype
        y = torch.empty(x.shape, dtype=torch.bfloat16 if yd == BF16 else torch.float32, device=x.device)
        check(load().lgcn_spmm_csr_drop(self.handle, tp(x), xd, tp(y), yd, int(x.shape[1]), float(keep_prob), int(seed) & (2 ** 64 - 1),
                                        int(step), 1 if transposed else 0, current_stream()), "lgcn_spmm_csr_drop")
        return y

    def close(self):
        if getattr(self, "handle", None):
            load().lgcn_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
