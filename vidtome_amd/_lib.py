"""ctypes binding of libvidtome_hip.so (the C ABI declared in include/vidtome_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator) and the current HIP stream; every
function below passes raw device pointers + sizes to the library.  There is NO fallback: if the library
is missing or a call fails, a RuntimeError is raised.

torch must be imported before the library is loaded so that both bind the same HIP runtime
(libamdhip64.so.7 is resolved by SONAME against the copy torch already mapped).
"""
from __future__ import annotations

import ctypes
import functools
import math
import operator
import os
import struct
import threading
from typing import Optional, Tuple

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 2   # include/vidtome_hip.h VTM_ABI_VERSION (2: flags_out of the filtered matchers is 8 int32)
LIB_PATH = os.environ.get("VIDTOME_HIP_LIB") or os.path.join(_HERE, "lib", "libvidtome_hip.so")

VTM_F32, VTM_F16, VTM_BF16 = 0, 1, 2
ROW_PAD, K_PAD = 256, 32
PROBS_MAX_KEYS, PROBS_MAX_HEADS = 256, 40   # what vtm_attention_probs takes (csrc/attention_probs.hip)

_DT = {torch.float32: VTM_F32, torch.float16: VTM_F16, torch.bfloat16: VTM_BF16}

_vp, _i64, _int, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
_u64, _u32 = ctypes.c_uint64, ctypes.c_uint32
_lib: Optional[ctypes.CDLL] = None

_SIGNATURES = {
    "vtm_version": ([], _int),
    "vtm_last_error": ([], ctypes.c_char_p),
    "vtm_build_ablations": ([], _int),
    "vtm_pad_rows": ([_i64], _i64),
    "vtm_pad_k": ([_i64], _i64),
    "vtm_normalize_gather": ([_vp, _i64, _vp, _i64, _int, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _vp], _int),
    "vtm_match": ([_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp], _int),
    "vtm_match_masked_ws_bytes": ([_i64, _i64, _i64], ctypes.c_size_t),
    "vtm_match_masked": ([_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _int, _vp, _i64, _i64, _vp, _vp, _f32, _vp,
                          ctypes.c_size_t, _vp, _vp], _int),
    "vtm_match_filtered_ws_bytes": ([_i64, _i64, _i64, _i64, _int], ctypes.c_size_t),
    "vtm_match_filtered": ([_vp, _i64, _vp, _i64, _int, _i64, _i64, _vp, _i64, _vp, _i64, _int, _vp, ctypes.c_size_t,
                            _vp, _vp, _vp], _int),
    "vtm_match_filtered_plan": ([_vp, _i64, _vp, _i64, _int, _i64, _i64, _vp, _i64, _vp, _i64, _int, _vp, ctypes.c_size_t,
                                 _vp, _vp, _i64, _i64, _vp, _vp, _int, _vp], _int),
    "vtm_match_filtered_ordered": ([_vp, _i64, _vp, _i64, _int, _i64, _i64, _vp, _i64, _vp, _i64, _int, _vp, ctypes.c_size_t,
                                    _vp, _vp, _i64, _i64, _vp, _vp, _int, _vp, _vp, _vp], _int),
    "vtm_position_order_counter_ints": ([_i64, _i64], ctypes.c_size_t),
    "vtm_position_order_ws_bytes": ([_i64, _i64, _i64, _i64], ctypes.c_size_t),
    "vtm_position_order": ([_vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp,
                            _vp, _vp, _int, _vp], _int),
    "vtm_match_filtered_seeded": ([_vp, _i64, _vp, _i64, _int, _i64, _i64, _vp, _i64, _vp, _i64, _int, _vp, ctypes.c_size_t,
                                   _vp, _vp, _i64, _i64, _vp, _vp, _vp], _int),
    "vtm_anchor_pos": ([_vp, _i64, _i64, _i64, _i64, _vp, _i64, _vp, _vp], _int),
    "vtm_decode_best": ([_vp, _i64, _vp, _vp, _vp], _int),
    "vtm_sort_ws_bytes": ([_i64, _i64], ctypes.c_size_t),
    "vtm_sort_desc": ([_vp, _i64, _i64, _vp, _vp, ctypes.c_size_t, _vp], _int),
    "vtm_partition_counts": ([_i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _int),
    "vtm_partition_local": ([_vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp], _int),
    "vtm_partition_global": ([_vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp], _int),
    "vtm_partition_2d": ([_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp], _int),
    "vtm_plan_apply": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp,
                        _vp, _vp], _int),
    "vtm_compose": ([_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp], _int),
    "vtm_gather_rows": ([_vp, _i64, _vp, _i64, _int, _i64, _i64, _vp, _i64, _vp, _i64, _vp], _int),
    "vtm_unmerge_add": ([_vp, _i64, _vp, _vp, _int, _i64, _i64, _i64, _vp, _vp], _int),
    "vtm_merge_reduce": ([_vp, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _i64, _i64, _vp], _int),
    "vtm_attention": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _f32,
                       _int, _vp, ctypes.c_size_t, _vp], _int),
    "vtm_attention_ws_bytes": ([_i64, _i64, _i64, _i64, _i64], ctypes.c_size_t),
    "vtm_attention_ws_bytes_dtype": ([_int, _i64, _i64, _i64, _i64, _i64], ctypes.c_size_t),
    "vtm_attention_kv": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                          _f32, _int, _vp, ctypes.c_size_t, _vp], _int),
    "vtm_attention_kv_sets": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                               _int, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_f32), _vp], _int),
    "vtm_attention_kv_sets_masked": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _f32,
                                      _int, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_f32),
                                      ctypes.POINTER(_int), _vp, _i64, _i64, _vp], _int),
    "vtm_attention_kv_sets_src": ([_vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64,
                                   _i64, _f32, _int, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_f32),
                                   ctypes.POINTER(_int), _vp], _int),
    "vtm_cross_edit_values": ([_vp, _i64, _i64, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp], _int),
    "vtm_attention_kv_bias": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                               _f32, _vp, _i64, _i64, _vp], _int),
    "vtm_frame_order_ws_bytes": ([_i64, _i64, _i64], ctypes.c_size_t),
    "vtm_frame_order": ([_vp, _i64, _vp, _i64, _i64, _i64, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp], _int),
    "vtm_attention_kv_segments": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _vp, _i64, _i64, _i64, _i64, _i64,
                                   _i64, _f32, _vp], _int),
    "vtm_attention_probs": ([_vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _vp, _i64,
                             _i64, _vp], _int),
    "vtm_attention_word_map": ([_vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _vp, _i64, _i64, _vp, _i64,
                                _i64, _vp, _i64, _vp, _int, _vp], _int),
    "vtm_local_blend": ([_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _int, _i64, _i64, _i64, _int, _f32, _vp, _vp], _int),
    "vtm_attention_key_mass_ws_bytes": ([_i64, _i64, _i64], ctypes.c_size_t),
    "vtm_attention_key_mass": ([_vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _vp,
                                ctypes.c_size_t, _vp], _int),
    "vtm_sag_degrade": ([_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _int, _i64, _i64, _i64, _i64, _int, _f32, _f32,
                         ctypes.POINTER(_f32), _int, _f32, _vp, _vp, _vp], _int),
    "vtm_freeu_lanes": ([_i64], _int),
    "vtm_freeu_ws_bytes": ([_i64, _i64, _int], ctypes.c_size_t),
    "vtm_freeu": ([_vp, _int, _i64, _i64, _i64, _i64, _i64, _f32, _f32, _int, _vp, ctypes.c_size_t, _vp], _int),
    "vtm_attention_kv_bounded": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                  _f32, _vp, _vp, ctypes.c_size_t, _vp], _int),
    "vtm_attention_kv_shared_bounded": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                         _f32, _int, _vp, _vp, ctypes.c_size_t, _vp], _int),
    "vtm_attention_kv_bounded_ws_bytes": ([_i64, _i64, _i64, _i64, _i64], ctypes.c_size_t),
    "vtm_attention_kv_bounded_ws_bytes_dtype": ([_int, _i64, _i64, _i64, _i64, _i64], ctypes.c_size_t),
    "vtm_anchor_maps": ([_vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp], _int),
    "vtm_transpose_cols": ([_vp, _i64, _int, _i64, _i64, _i64, _vp, _i64, _vp], _int),
    "vtm_fold_keys_ws_bytes": ([_i64, _i64, _i64], ctypes.c_size_t),
    "vtm_fold_keys": ([_vp, _i64, _i64, _i64, _vp, _i64, _i64, _int, _vp, ctypes.c_size_t, _vp, _vp, _i64, _vp, _vp], _int),
    "vtm_attention_kv_folded": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                 _f32, _vp, _vp, _vp, _i64, _vp, ctypes.c_size_t, _vp], _int),
    "vtm_compact_queries_ws_bytes": ([_i64, _i64], ctypes.c_size_t),
    "vtm_compact_queries": ([_vp, _i64, _i64, _i64, _i64, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp], _int),
    "vtm_panel_rows": ([_i64], _i64),
    "vtm_to_panels": ([_vp, _int, _i64, _i64, _vp, _vp, _i64, _vp], _int),
    "vtm_layernorm_panels": ([_vp, _vp, _vp, _int, _i64, _i64, _f32, _vp, _i64, _vp], _int),
    "vtm_gather_panels": ([_vp, _i64, _vp, _i64, _int, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp], _int),
    "vtm_ff_geglu": ([_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _int, _vp, _vp], _int),
    "vtm_linear_panels": ([_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _int, _vp, _i64, _vp], _int),
    "vtm_cfg_ddim": ([_vp, _vp, _vp, _int, _i64, _f32, _f32, _f32, _f32, _f32, _vp, _vp, _vp], _int),
    "vtm_guided_step": ([_vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _vp, _int, _f32, _f32, _f32, _f32, _f32, _f32, _f32,
                         _vp, _vp, _vp, _vp], _int),
    "vtm_solver_step": ([_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, ctypes.POINTER(_f32), _i64, _vp, _int, _f32, _f32, _f32,
                         _f32, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _vp, _vp], _int),
    "vtm_invert_step": ([_vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, ctypes.POINTER(_f32), _i64, _vp, _int, _f32, _f32, _f32, _f32,
                         _f32, _f32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp], _int),
    "vtm_noise_levels": ([_vp, _vp, _vp, _int, _i64, _i64, _vp], _int),
    "vtm_frame_noise": ([_vp, _int, _i64, _i64, _i64, _vp, _i64, _u64, _u32, _u32, _vp], _int),
    "vtm_philox_bits": ([_vp, _i64, _u64, _vp, _vp], _int),
    "vtm_guided_step_keyed": ([_vp, _vp, _u64, _u32, _u32, _i64, _int, _i64, _i64, _i64, _i64, _i64, _vp, _int, _f32, _f32, _f32,
                               _f32, _f32, _f32, _f32, _vp, _vp, _vp, _vp], _int),
    "vtm_solver_step_keyed": ([_vp, _vp, _u64, _u32, _u32, _i64, _vp, _vp, _int, _i64, _i64, _i64, ctypes.POINTER(_f32), _i64, _vp,
                               _int, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _vp, _vp], _int),
    "vtm_semantic_guidance": ([_vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _i64, ctypes.POINTER(ctypes.c_int32),
                               ctypes.POINTER(_f32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
                               ctypes.POINTER(_f32), ctypes.POINTER(_f32), ctypes.POINTER(ctypes.c_int32), _vp, _vp, _i64, _vp,
                               _f32, _f32, _int, _vp, _vp, _vp], _int),
    "vtm_layernorm": ([_vp, _vp, _vp, _int, _i64, _i64, _f32, _vp, _vp], _int),
    "vtm_layernorm_gather": ([_vp, _vp, _vp, _int, _i64, _i64, _i64, _vp, _i64, _f32, _vp, _i64, _vp], _int),
    "vtm_geglu": ([_vp, _int, _i64, _i64, _vp, _vp], _int),
    "vtm_linear_rows": ([_vp, _i64, _vp, _i64, _int, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64,
                         _int, _vp], _int),
    "vtm_lora_fold": ([_vp, _int, _vp, _vp, _i64, _i64, _i64, _vp, _vp], _int),
    "vtm_dora_norms": ([_vp, _int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp], _int),
    "vtm_dora_fold": ([_vp, _int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp], _int),
    "vtm_loha_delta": ([_vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp], _int),
    "vtm_lokr_delta": ([_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp], _int),
    "vtm_delta_fold": ([_vp, _int, _vp, _i64, _i64, _vp, _vp], _int),
    "vtm_groupnorm_silu": ([_vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _f32, _int, _vp, _vp], _int),
    "vtm_resnet_tail": ([_vp, _vp, _int, _i64, _i64, _i64, _i64, ctypes.c_double, _vp, _vp], _int),
    "vtm_linear_f32": ([_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _int, _vp, _vp, _int, _i64,
                        _i64, _int, _vp], _int),
    "vtm_residual_record": ([_vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _vp], _int),
    "vtm_residual_replay": ([_vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _vp, _vp], _int),
    "vtm_residual_replay_layernorm": ([_vp, _vp, _vp, _vp, _vp, _vp, _f32, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _i64,
                                       _vp], _int),
}


def exported_symbols():
    """Names include/vidtome_hip.h declares (used by the CPU test that checks the .so exports them)."""
    return sorted(_SIGNATURES)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m vidtome_amd.build` (hipcc, gfx950). "
                "vidtome_amd has no CPU / eager fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(L, name)   # AttributeError here = the .so is stale w.r.t. the header
            fn.argtypes = argtypes
            fn.restype = restype
        if L.vtm_version() != ABI_VERSION:
            raise RuntimeError("libvidtome_hip.so ABI version mismatch")
        if L.vtm_build_ablations() != 0 and os.environ.get("VIDTOME_ALLOW_ABLATED") != "1":
            # an experiment build (csrc/ablate.h) computes wrong results by construction: only tools/ may load one, knowingly
            raise RuntimeError(f"{LIB_PATH} was built with ablation switches (mask {L.vtm_build_ablations():#x}); "
                               "set VIDTOME_ALLOW_ABLATED=1 to load it for a timing experiment")
        _lib = L
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().vtm_last_error()
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def _stream() -> int:
    """Raw HIP stream the launch goes to: torch's current stream of the CURRENT device -- every wrapper below runs
    under `_on_device`, which makes the operands' device the current one first."""
    return torch.cuda.current_stream().cuda_stream


def _on_device(fn):
    """Run the wrapper with its first tensor argument's device as the current HIP device (a model moved to cuda:1
    in a process whose current device is cuda:0 must launch on cuda:1's stream, not enqueue foreign pointers on
    cuda:0).  The common case -- already current -- costs one integer comparison."""
    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        dev = next((a.device if isinstance(a, torch.Tensor) else a for a in args
                    if isinstance(a, (torch.Tensor, torch.device))), None)
        if dev is None or dev.type != "cuda" or dev.index is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev.index):
            return fn(*args, **kwargs)
    return guarded


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_WS: dict = {}
_WS_LOCK = threading.Lock()


def _workspace(tag: str, nbytes: int, device: torch.device) -> torch.Tensor:
    """Scratch memory of a call, cached per (device, stream, purpose) and grown on demand: calls on one stream are
    ordered, so the next user of the buffer starts after the previous one finished -- no allocator round trip per
    call (a block makes ~40 of them).  The library itself stays stateless: it is handed the pointer and the size.
    The host thread is part of the key: two threads launching on the same stream never share a buffer (their launches
    are not ordered against each other by anything the caller can rely on).  `remove_patch` drops the cache."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, tag, threading.get_ident())
    buf = _WS.get(key)                     # (a thread only ever reads / replaces its OWN keys outside the lock)
    if buf is None or buf.numel() < nbytes:
        new = torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)
        with _WS_LOCK:                     # insertion + clean-up mutate the dict other threads iterate
            if buf is None:
                # a new (thread, stream, purpose): the moment to let go of the buffers of threads that no longer exist
                alive = {t.ident for t in threading.enumerate()}
                for k in [k for k in list(_WS) if k[3] not in alive]:
                    _WS.pop(k, None)
            _WS[key] = new
        buf = new
    return buf


def release_workspaces() -> None:
    """Drop the cached scratch buffers (they are re-created on demand)."""
    with _WS_LOCK:
        _WS.clear()
        _ZEROED.clear()


def _req(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (vidtome_amd has no CPU path)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t


def dtype_code(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise RuntimeError(f"unsupported dtype {t.dtype}") from None


def pad_rows(n: int) -> int:
    return (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD


def pad_k(c: int) -> int:
    return (c + K_PAD - 1) // K_PAD * K_PAD


# --------------------------------------------------------------------------------------------------
@_on_device
def normalize_gather(x0: torch.Tensor, x1: Optional[torch.Tensor], rows: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """rows (B, n) int32 pool ids -> (operand (B, C_pad/8, 2, n_pad, 4) fp32 k-panels, norms (B, n))."""
    _req(x0, "x0"), _req(rows, "rows")
    B, P0, C = x0.shape
    P1 = 0 if x1 is None else _req(x1, "x1").shape[1]
    n = rows.shape[1]
    n_pad, C_pad = pad_rows(n), pad_k(C)
    out = torch.empty((B, C_pad // 8, 2, n_pad, 4), dtype=torch.float32, device=x0.device)
    norms = torch.empty((B, max(n, 1)), dtype=torch.float32, device=x0.device)
    _check(lib().vtm_normalize_gather(_ptr(x0), P0, _ptr(x1), P1, dtype_code(x0), B, C, _ptr(rows), n,
                                      _ptr(norms), _ptr(out), n_pad, C_pad, _stream()), "vtm_normalize_gather")
    return out, norms


@_on_device
def match(a: torch.Tensor, b: torch.Tensor, Ns: int, Nd: int, align: bool) -> torch.Tensor:
    """Packed (orderable(max) << 32 | ~argmax) per src row: (B, Ns) or (1, Ns) when aligned (int64 bits)."""
    B, G, _, Ns_pad, _ = a.shape
    C_pad, Nd_pad = G * 8, b.shape[3]
    best = torch.empty((1 if align else B, Ns), dtype=torch.int64, device=a.device)
    _check(lib().vtm_match(_ptr(a), _ptr(b), B, Ns, Nd, Ns_pad, Nd_pad, C_pad, int(align), _ptr(best), _stream()),
           "vtm_match")
    return best


def _f32_round(v: float) -> float:
    return struct.unpack("<f", struct.pack("<f", v))[0]


def _f32_step(v: float, up: bool) -> float:
    """The neighbour of the non-negative finite fp32 ``v`` (towards +inf / towards 0)."""
    bits = struct.unpack("<I", struct.pack("<f", v))[0]
    return struct.unpack("<f", struct.pack("<I", bits + 1 if up else bits - 1))[0]


_F32_MAX = struct.unpack("<f", struct.pack("<I", 0x7F7FFFFF))[0]


def mask_threshold(rec_field: float) -> float:
    """T of vtm_match_masked: the largest fp32 t with fl32(sqrt(t)) <= fl32(rec_field), so that ``s > T`` on the squared
    distance is the reference's ``torch.norm(...) > rec_field`` (merge.py:235; torch compares an fp32 tensor with a Python
    number in fp32).  -inf for a negative field (every distance exceeds it), +inf for NaN / +inf (none does).  Pure host
    arithmetic: sqrt in double and one rounding equal the correctly rounded fp32 sqrt (53 >= 2 * 24 + 2)."""
    rec = float(rec_field)
    if rec != rec:
        return math.inf
    rec = math.copysign(math.inf, rec) if abs(rec) > _F32_MAX * (1 + 2.0 ** -25) else _f32_round(rec)
    if rec < 0:
        return -math.inf
    if rec == math.inf:
        return math.inf
    ok = lambda t: _f32_round(math.sqrt(t)) <= rec
    sq = rec * rec                                   # exact in double
    t = _F32_MAX if sq >= _F32_MAX else _f32_round(sq)
    while t > 0.0 and not ok(t):
        t = _f32_step(t, False)
    while t < _F32_MAX and ok(_f32_step(t, True)):
        t = _f32_step(t, True)
    return t


@_on_device
def match_masked(a: torch.Tensor, b: torch.Tensor, Ns: int, Nd: int, align: bool, coord: torch.Tensor,
                 a_rows: torch.Tensor, b_rows: torch.Tensor, T: float) -> torch.Tensor:
    """``match`` with the receptive field: coord (B or 1, P, 4) fp32 coordinate pool, a_rows (B, Ns) / b_rows (B, Nd) int32
    rows of it, T = mask_threshold(rec_field).  Same packed keys; see include/vidtome_hip.h."""
    _req(coord, "coord"), _req(a_rows, "a_rows"), _req(b_rows, "b_rows")
    B, G, _, Ns_pad, _ = a.shape
    C_pad, Nd_pad = G * 8, b.shape[3]
    if coord.dtype != torch.float32 or coord.dim() != 3 or coord.shape[2] != 4 or coord.shape[0] not in (1, B):
        raise RuntimeError(f"match_masked: the coordinate pool must be (B or 1, P, 4) fp32, got {tuple(coord.shape)} {coord.dtype}")
    if a_rows.dtype != torch.int32 or b_rows.dtype != torch.int32 or a_rows.shape != (B, Ns) or b_rows.shape != (B, Nd):
        raise RuntimeError("match_masked: a_rows / b_rows must be (B, Ns) / (B, Nd) int32")
    best = torch.empty((1 if align else B, Ns), dtype=torch.int64, device=a.device)
    nbytes = lib().vtm_match_masked_ws_bytes(B, Ns_pad, Nd_pad)
    ws = _workspace("match_masked", nbytes, a.device)
    _check(lib().vtm_match_masked(_ptr(a), _ptr(b), B, Ns, Nd, Ns_pad, Nd_pad, C_pad, int(align), _ptr(coord), coord.shape[0],
                                  coord.shape[1], _ptr(a_rows), _ptr(b_rows), T, _ptr(ws), nbytes, _ptr(best), _stream()),
           "vtm_match_masked")
    return best


MATCH_ONE_LAUNCH, MATCH_SCOUT_RANGE = 0, 1         # include/vidtome_hip.h: VTM_MATCH_*


@_on_device
def match_filtered(x0: torch.Tensor, x1: Optional[torch.Tensor], a_rows: torch.Tensor, b_rows: torch.Tensor,
                   align: bool, want_flag: bool = False, seed=None, mode: int = MATCH_ONE_LAUNCH,
                   stats_host: Optional[torch.Tensor] = None, order=None, scout_steps: int = 0):
    """Same packed result as normalize_gather x2 + match, through the fp16-filter / fp32-refine path.  ``seed`` (optional,
    never changes the result): (tokens per frame N, L = pool rows that are chunk tokens, pos1 (B, P1) int32 positions of the
    x1 rows or None, table (B, N) int32 position -> dst index or None for identity) -- every src row then starts from the
    score of the dst row at its own token position.  ``mode`` = the launch plan (MATCH_ONE_LAUNCH / MATCH_SCOUT_RANGE: a scout
    launch + the filter over the spans of live dst tiles, for levels with position-ordered rows; same bits;
    include/vidtome_hip.h, vtm_match_filtered_plan).  ``stats_host``: a PINNED host tensor of 8 int32 that receives the
    call's counters asynchronously (flags_out of the C ABI) -- what merge.MatchPlanner steers by; ``want_flag`` returns them
    as a device tensor instead.  ``order`` = (a_order, b_order) from `position_order`: a_rows / b_rows are then its SORTED lists
    and the result is reported (and ties are broken) in the original indexing -- the same bits as the call on the unsorted
    lists (vtm_match_filtered_ordered; aligned calls: lists from a ``shared`` position_order).  ``scout_steps`` (scout + range plan): the scout tests after that many
    64-channel steps instead of the filter's own test depth (VTM_MATCH_SCOUT_STEPS; 0 = the filter's depth)."""
    _req(x0, "x0"), _req(a_rows, "a_rows"), _req(b_rows, "b_rows")
    B, P0, C = x0.shape
    P1 = 0 if x1 is None else _req(x1, "x1").shape[1]
    Ns, Nd = a_rows.shape[1], b_rows.shape[1]
    nbytes = lib().vtm_match_filtered_ws_bytes(B, C, Ns, Nd, int(align))
    ws = _workspace("match", nbytes, x0.device)
    best = torch.empty((1 if align else B, Ns), dtype=torch.int64, device=x0.device)
    # whole-call escape, unusable norm seen, escaped rows, refined pairs, blocks tested, blocks alive, (internal), scout's
    # live wave tiles
    flag = torch.zeros((8,), dtype=torch.int32, device=x0.device) if want_flag else None
    flags_out = _ptr(flag)
    if flag is None and stats_host is not None:
        if not (stats_host.is_pinned() and stats_host.dtype == torch.int32 and stats_host.numel() >= 8):
            raise RuntimeError("match_filtered: stats_host must be a pinned int32 tensor of 8 elements")
        flags_out = stats_host.data_ptr()
    mode = int(mode) | ((int(scout_steps) & 0xff) << 8)
    sN = sL = 0
    pos1 = table = None
    if seed is not None and SEED_MATCHER:
        sN, sL, pos1, table = seed
        if pos1 is not None and (pos1.dtype != torch.int32 or tuple(pos1.shape) != (B, P1) or not pos1.is_contiguous()):
            raise RuntimeError("match_filtered: seed positions must be a contiguous (B, P1) int32 tensor")
        if table is not None and (table.dtype != torch.int32 or tuple(table.shape) != (B, sN) or not table.is_contiguous()):
            raise RuntimeError("match_filtered: the seed table must be a contiguous (B, N) int32 tensor")
    if order is not None:
        a_order, b_order = order
        for o, n, name in ((a_order, Ns, "a_order"), (b_order, Nd, "b_order")):
            if o.dtype != torch.int32 or tuple(o.shape) != (B, n) or not o.is_contiguous() or not o.is_cuda:
                raise RuntimeError(f"match_filtered: {name} must be a contiguous (B, {n}) int32 device tensor")
        _check(lib().vtm_match_filtered_ordered(_ptr(x0), P0, _ptr(x1), P1, dtype_code(x0), B, C, _ptr(a_rows), Ns,
                                                _ptr(b_rows), Nd, int(align), _ptr(ws), nbytes, _ptr(best), flags_out, int(sL), int(sN),
                                                _ptr(pos1), _ptr(table), int(mode), _ptr(a_order), _ptr(b_order), _stream()),
               "vtm_match_filtered_ordered")
        return (best, flag) if want_flag else best
    _check(lib().vtm_match_filtered_plan(_ptr(x0), P0, _ptr(x1), P1, dtype_code(x0), B, C, _ptr(a_rows), Ns,
                                         _ptr(b_rows), Nd, int(align), _ptr(ws), nbytes, _ptr(best), flags_out,
                                         int(sL), int(sN), _ptr(pos1), _ptr(table), int(mode), _stream()),
           "vtm_match_filtered_plan")
    return (best, flag) if want_flag else best


POSITION_ORDER_MAX_N = 16360        # include/vidtome_hip.h: VTM_POSITION_ORDER_MAX_N
_ZEROED: dict = {}


def _zeroed_counters(n_ints: int, device: torch.device) -> torch.Tensor:
    """The counter block of vtm_position_order: zero when a call starts, zero again when it has run -- allocated (zeroed)
    once per (device, stream, thread) like the scratch buffers, re-allocated when a larger one is needed."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, threading.get_ident())
    buf = _ZEROED.get(key)
    if buf is None or buf.numel() < n_ints:
        buf = torch.zeros((max(int(n_ints), 16),), dtype=torch.int32, device=device)
        with _WS_LOCK:
            _ZEROED[key] = buf
    return buf


@_on_device
def position_order(a_rows: torch.Tensor, b_rows: torch.Tensor, L: int, N: int, pos1: Optional[torch.Tensor], P0: int,
                   want_table: bool = True, shared: bool = False):
    """Both row lists of a matcher call sorted by token position (vtm_position_order, include/vidtome_hip.h):
    -> (a_sorted, a_order, b_sorted, b_order, table).  Position of pool row r: r % N below L, pos1[b, r - P0] for the rows of
    x1 (``pos1`` (B, P1) int32 or None).  ``shared`` (aligned matching): ONE order, sample 0's, for every sample's lists."""
    _req(a_rows, "a_rows"), _req(b_rows, "b_rows")
    B, Ns = a_rows.shape
    Nd = b_rows.shape[1]
    P1 = 0
    if pos1 is not None:
        if pos1.dtype != torch.int32 or pos1.dim() != 2 or pos1.shape[0] != B or not pos1.is_contiguous():
            raise RuntimeError("position_order: positions must be a contiguous (B, P1) int32 tensor")
        P1 = pos1.shape[1]
    dev = a_rows.device
    counters = _zeroed_counters(lib().vtm_position_order_counter_ints(B, N), dev)
    nbytes = lib().vtm_position_order_ws_bytes(B, Ns, Nd, N)
    ws = _workspace("order", nbytes, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    a_sorted, a_order = torch.empty((B, Ns), **i32), torch.empty((B, Ns), **i32)
    b_sorted, b_order = torch.empty((B, Nd), **i32), torch.empty((B, Nd), **i32)
    table = torch.empty((B, N), **i32) if want_table else None
    _check(lib().vtm_position_order(_ptr(a_rows), Ns, _ptr(b_rows), Nd, B, int(L), int(N), _ptr(pos1), int(P0), P1,
                                    _ptr(counters), _ptr(ws), nbytes, _ptr(a_sorted), _ptr(a_order), _ptr(b_sorted),
                                    _ptr(b_order), _ptr(table), int(shared), _stream()), "vtm_position_order")
    return a_sorted, a_order, b_sorted, b_order, table


@_on_device
def decode_best(best: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    nm = torch.empty(best.shape, dtype=torch.float32, device=best.device)
    ni = torch.empty(best.shape, dtype=torch.int32, device=best.device)
    _check(lib().vtm_decode_best(_ptr(best), best.numel(), _ptr(nm), _ptr(ni), _stream()), "vtm_decode_best")
    return nm, ni


@_on_device
def sort_desc(best: torch.Tensor) -> torch.Tensor:
    rows, n = best.shape
    perm = torch.empty((rows, n), dtype=torch.int32, device=best.device)
    nbytes = lib().vtm_sort_ws_bytes(rows, n)
    ws = _workspace("sort", nbytes, best.device)
    _check(lib().vtm_sort_desc(_ptr(best), rows, n, _ptr(perm), _ptr(ws), nbytes, _stream()), "vtm_sort_desc")
    return perm


def partition_counts(N_in: int, unm_pre: int, tnum: int, ts: int, randf: int) -> Tuple[int, int]:
    ns, nd = _i64(0), _i64(0)
    _check(lib().vtm_partition_counts(N_in, unm_pre, tnum, ts, randf, ctypes.byref(ns), ctypes.byref(nd)),
           "vtm_partition_counts")
    return int(ns.value), int(nd.value)


@_on_device
def partition_local(cur: Optional[torch.Tensor], B: int, N_in: int, unm_pre: int, tnum: int, ts: int,
                    randf: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    Ns, Nd = partition_counts(N_in, unm_pre, tnum, ts, randf)
    i32 = dict(dtype=torch.int32, device=device)
    a_pos, b_pos = torch.empty((Ns,), **i32), torch.empty((Nd,), **i32)
    a_rows, b_rows = torch.empty((B, Ns), **i32), torch.empty((B, Nd), **i32)
    _check(lib().vtm_partition_local(_ptr(cur), B, N_in, unm_pre, tnum, ts, randf, _ptr(a_pos), _ptr(b_pos),
                                     _ptr(a_rows), _ptr(b_rows), Ns, Nd, _stream()), "vtm_partition_local")
    return a_pos, b_pos, a_rows, b_rows


@_on_device
def partition_2d(device, h: int, w: int, sx: int, sy: int, draws: Optional[torch.Tensor]
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(a_idx (N - hsy * wsx,), b_idx (hsy * wsx,)) int32 of bipartite_soft_matching_random2d (merge.py:493-528), both in
    ascending token order; ``draws`` = the (hsy * wsx,) int32 cell draws on the device, None = no_rand."""
    h, w, sx, sy = int(h), int(w), int(sx), int(sy)
    if min(h, w, sx, sy) <= 0 or sx > w or sy > h:
        raise ValueError(f"partition_2d: strides ({sx}, {sy}) must lie in [1, w] x [1, h] of a {w} x {h} frame")
    Nd = (h // sy) * (w // sx)
    if draws is not None and (draws.dtype != torch.int32 or draws.numel() != Nd or not draws.is_contiguous()
                              or not draws.is_cuda):
        raise RuntimeError(f"partition_2d: the draws must be {Nd} contiguous int32 on the GPU")
    i32 = dict(dtype=torch.int32, device=device)
    a_idx, b_idx = torch.empty((h * w - Nd,), **i32), torch.empty((Nd,), **i32)
    _check(lib().vtm_partition_2d(h, w, sx, sy, _ptr(draws), _ptr(b_idx), _ptr(a_idx) or None, _stream()),
           "vtm_partition_2d")
    return a_idx, b_idx


@_on_device
def anchor_pos(amap: Optional[torch.Tensor], B: int, M: int, L: int, tokens: int, old_pos: Optional[torch.Tensor],
               device) -> torch.Tensor:
    """Token positions (B, M) int32 of a new anchor set = pool[amap] (amap None: the first M pool rows), pool = [chunk of L
    rows | old anchors with positions old_pos]; -1 = unknown."""
    out = torch.empty((B, M), dtype=torch.int32, device=device)
    Mg = 0 if old_pos is None else old_pos.shape[1]
    _check(lib().vtm_anchor_pos(_ptr(amap), B, M, L, tokens, _ptr(old_pos), Mg, _ptr(out), _stream()), "vtm_anchor_pos")
    return out


@_on_device
def anchor_maps(inv_g: torch.Tensor, off: int, new_cur: torch.Tensor, Ml: int, L: int, tokens: int,
                old_pos: Optional[torch.Tensor], want_pos: bool) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(loc, amap, pos) behind a global level: merged position of every local token, pool row of every new anchor, and
    (``want_pos``) its token position; see include/vidtome_hip.h."""
    _req(inv_g, "inv_g"), _req(new_cur, "new_cur")
    B, N_in = inv_g.shape
    i32 = dict(dtype=torch.int32, device=inv_g.device)
    loc, amap = torch.empty((B, Ml), **i32), torch.empty((B, Ml), **i32)
    pos = torch.empty((B, Ml), **i32) if want_pos else None
    Mg = 0 if old_pos is None else old_pos.shape[1]
    _check(lib().vtm_anchor_maps(_ptr(inv_g), N_in, off, _ptr(new_cur), new_cur.shape[1], B, Ml, L, tokens if want_pos else 0,
                                 _ptr(old_pos), Mg, _ptr(loc), _ptr(amap), _ptr(pos), _stream()), "vtm_anchor_maps")
    return loc, amap, pos


@_on_device
def partition_global(cur_local: torch.Tensor, anchor_base: int, Mg: int, local_is_src: bool, seed_table: Optional[torch.Tensor] = None,
                     tokens: int = 0, anchor_positions: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``seed_table`` (B, tokens) int32 (optional) is filled with position -> dst index for the matcher's seeds."""
    B, Ml = cur_local.shape
    src_len = Ml if local_is_src else Mg
    Nd = Ml + Mg - src_len
    i32 = dict(dtype=torch.int32, device=cur_local.device)
    a_pos, b_pos = torch.empty((src_len,), **i32), torch.empty((Nd,), **i32)
    a_rows, b_rows = torch.empty((B, src_len), **i32), torch.empty((B, Nd), **i32)
    _check(lib().vtm_partition_global(_ptr(cur_local), B, Ml, anchor_base, Mg, int(local_is_src), _ptr(a_pos),
                                      _ptr(b_pos), _ptr(a_rows), _ptr(b_rows), _ptr(seed_table), int(tokens),
                                      _ptr(anchor_positions), _stream()), "vtm_partition_global")
    return a_pos, b_pos, a_rows, b_rows


@_on_device
def plan_apply(best, perm, a_pos, b_pos, a_rows, b_rows, r: int, align: bool, want_indices: bool):
    B, Ns = a_rows.shape
    Nd = b_rows.shape[1]
    N_in, U = Ns + Nd, Ns - r
    i32 = dict(dtype=torch.int32, device=a_rows.device)
    new_cur = torch.empty((B, U + Nd), **i32)
    inv = torch.empty((B, N_in), **i32)
    unm_idx = torch.empty((B, U), **i32) if want_indices else None
    src_idx = torch.empty((B, r), **i32) if want_indices else None
    dst_idx = torch.empty((B, r), **i32) if want_indices else None
    _check(lib().vtm_plan_apply(_ptr(best), _ptr(perm), _ptr(a_pos), _ptr(b_pos), _ptr(a_rows), _ptr(b_rows), B,
                                N_in, Ns, Nd, r, int(align), _ptr(new_cur), _ptr(inv), _ptr(unm_idx),
                                _ptr(src_idx), _ptr(dst_idx), _stream()), "vtm_plan_apply")
    return new_cur, inv, unm_idx, src_idx, dst_idx


@_on_device
def compose(inv_acc: Optional[torch.Tensor], inv_level: torch.Tensor, n: int, offset: int = 0) -> torch.Tensor:
    B, level_len = inv_level.shape
    out = torch.empty((B, n), dtype=torch.int32, device=inv_level.device)
    _check(lib().vtm_compose(_ptr(inv_acc), _ptr(inv_level), B, n, level_len, offset, _ptr(out), _stream()),
           "vtm_compose")
    return out


@_on_device
def gather_rows(x0: torch.Tensor, x1: Optional[torch.Tensor], idx: torch.Tensor, pad_to: int = 1) -> torch.Tensor:
    """out (B, M_pad, C): rows [0, M) = pool[idx]; rows >= M (padding up to a multiple of pad_to) are zero."""
    _req(x0, "x0"), _req(idx, "map")
    B, P0, C = x0.shape
    P1 = 0 if x1 is None else _req(x1, "x1").shape[1]
    M = idx.shape[1]
    Mp = (M + pad_to - 1) // pad_to * pad_to
    out = (torch.zeros if Mp != M else torch.empty)((B, Mp, C), dtype=x0.dtype, device=x0.device)
    _check(lib().vtm_gather_rows(_ptr(x0), P0, _ptr(x1), P1, dtype_code(x0), B, C, _ptr(idx), M, _ptr(out), Mp,
                                 _stream()), "vtm_gather_rows")
    return out


REDUCE_MODES = {"sum": 0, "prod": 1, "mean": 2, "amax": 3, "amin": 4}      # torch.scatter_reduce's (merge.py:127-131)


@_on_device
def merge_reduce(x: torch.Tensor, src_rows: torch.Tensor, dst_rows: torch.Tensor, dst_idx: torch.Tensor, mode: str,
                 out: torch.Tensor, out_row0: int) -> torch.Tensor:
    """The reference's non-"replace" merge modes: fold row src_rows[b, i] of x into dst row dst_idx[b, i] (whose own row
    of x is dst_rows[b, j]) like ``scatter_reduce(..., reduce=mode, include_self=True)`` on the CPU, writing the Nd
    reduced rows to out[:, out_row0:out_row0 + Nd].  The pairs are sorted by destination with the library's own stable
    radix sort (index order survives inside a destination's segment -- that order is the summation order)."""
    if mode not in REDUCE_MODES:
        raise ValueError(f"merge mode {mode!r}: expected 'replace' or one of {sorted(REDUCE_MODES)}")
    _req(x, "x"), _req(src_rows, "src_rows"), _req(dst_rows, "dst_rows"), _req(dst_idx, "dst_idx"), _req(out, "out")
    B, N, C = x.shape
    r, Nd = src_rows.shape[1], dst_rows.shape[1]
    if r > 0:
        keys = ((-1 - dst_idx.long()) << 32).contiguous()       # high word = 0xffffffff - dst: "descending" = ascending dst
        order = sort_desc(keys)
        seg_dst = torch.gather(dst_idx, 1, order.long()).contiguous()
    else:
        order = seg_dst = dst_idx
    _check(lib().vtm_merge_reduce(_ptr(x), dtype_code(x), B, N, C, _ptr(src_rows), _ptr(dst_rows), _ptr(seg_dst), _ptr(order),
                                  r, Nd, REDUCE_MODES[mode], _ptr(out), out.shape[1], out_row0, _stream()), "vtm_merge_reduce")
    return out


@_on_device
def unmerge_add(y: torch.Tensor, inv: torch.Tensor, resid: Optional[torch.Tensor]) -> torch.Tensor:
    """out[b, i] = y[b, inv[b, i]] (+ resid[b, i]);  y is (B, Mp, C) (only rows < M are referenced)."""
    _req(y, "y"), _req(inv, "inv")
    B, Mp, C = y.shape
    L = inv.shape[1]
    out = torch.empty((B, L, C), dtype=y.dtype, device=y.device)
    if resid is not None:
        _req(resid, "resid")
        if resid.numel() != out.numel() or resid.dtype != y.dtype:
            raise RuntimeError("residual shape/dtype mismatch")
    _check(lib().vtm_unmerge_add(_ptr(y), Mp, _ptr(inv), _ptr(resid), dtype_code(y), B, L, C, _ptr(out), _stream()),
           "vtm_unmerge_add")
    return out


@_on_device
def transpose_cols(x: torch.Tensor, c0: int, C: int) -> torch.Tensor:
    """x (BF, N, ld) 16-bit, contiguous along the last axis -> (BF, C, Np) = columns [c0, c0 + C) channel-major, Np = N
    rounded up to 8 (zero-filled): the V^T operand of the attention core from a fused q | k | v projection."""
    _req(x, "x")
    BF, N, ld = x.shape
    if x.stride(2) != 1 or x.stride(1) != ld or x.stride(0) != N * ld or c0 % 8 or C % 8:
        raise RuntimeError("transpose_cols: dense (BF, N, ld) input, column window aligned to 8")
    Np = (N + 7) // 8 * 8
    out = torch.empty((BF, C, Np), dtype=x.dtype, device=x.device)
    _check(lib().vtm_transpose_cols(x.data_ptr() + c0 * x.element_size(), ld, dtype_code(x), BF, N, C, _ptr(out), Np, _stream()),
           "vtm_transpose_cols")
    return out


# A/B switch: seed the filtered matcher's running maxima from same-position guesses (profiles/r04_seeds.txt); results are
# identical either way
SEED_MATCHER = os.environ.get("VIDTOME_SEED", "1") != "0"

# A/B switch (profiles/r04_attention_split_all.txt): split every work item of a query-bounded attention launch in two
SPLIT_ALL_BOUNDED = os.environ.get("VIDTOME_ATT_SPLIT_ALL", "1") != "0"

# A/B switch: the anchors' exact duplicates enter attn1 as one key each (fold_keys / vtm_attention_kv_folded; d = 40 heads)
FOLD_KEYS = os.environ.get("VIDTOME_FOLD_KEYS", "1") != "0"


def _attention_ws(B: int, heads: int, Mq: int, Mk: int, d: int, device, dtype: torch.dtype = torch.float16):
    """Workspace for the split last round of an attention launch of `dtype` operands (None when the shape needs none;
    fp32 launches have plans of their own, the two 16-bit types share theirs)."""
    nb = int(lib().vtm_attention_ws_bytes_dtype(_DT[dtype], B, heads, Mq, Mk, d))
    if nb == 0:
        return None, 0
    return _workspace("attention", nb, device), nb


def _attention_out(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, Mq: int, Mkp: int, alloc: bool = True):
    """The operand checks every attention wrapper makes -- q (B, Mqp, C), k (B, Mkp, C), vt (B, C, ldvt) contiguous along
    the last axis, dense batch strides -- and its (B, Mqp, C) result: zeroed when there are pad rows behind Mq (no kernel
    writes them), else uninitialised."""
    B, Mqp, C = q.shape
    if q.stride(2) != 1 or k.stride(2) != 1 or vt.stride(2) != 1:
        raise RuntimeError("attention operands must be contiguous along their last axis")
    if q.stride(0) != Mqp * q.stride(1) or k.stride(0) != Mkp * k.stride(1) or vt.stride(0) != C * vt.stride(1):
        raise RuntimeError("attention operands must have dense batch strides")
    if not alloc:
        return None
    return (torch.zeros if Mqp != Mq else torch.empty)((B, Mqp, C), dtype=q.dtype, device=q.device)


def _out_like_q(who: str, out: torch.Tensor, q: torch.Tensor) -> None:
    if out.shape != q.shape or out.dtype != q.dtype or out.device != q.device or not out.is_contiguous():
        raise RuntimeError(f"{who}: out must be a contiguous tensor of q's shape, dtype and device")


_MODULE_PATH = " (fp32 models keep the module path)"


def _half_operands(who: str, q, k, vt=None, hint: str = "") -> None:
    """The side calls take fp16 / bf16 operands of one dtype (anything else, a non-tensor included, is refused here)."""
    ops = (q, k) if vt is None else (q, k, vt)
    if not all(isinstance(t, torch.Tensor) for t in ops) or q.dtype not in (torch.float16, torch.bfloat16) \
            or any(t.dtype != q.dtype for t in ops):
        raise RuntimeError(f"{who}: {'q and k' if vt is None else 'q, k and vt'} must share one of fp16 / bf16{hint}")


def _kv_shapes(who: str, q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor):
    """(B, Mqp, C, Mkp) of q (B, Mqp, C), k (B, Mkp, C) and vt (B, C, ldvt)."""
    B, Mqp, C = q.shape
    if k.shape[0] != B or vt.shape[0] != B or k.shape[2] != C or vt.shape[1] != C:
        raise RuntimeError(f"{who}: k must be (B, Mkp, C) and vt (B, C, ldvt)")
    return B, Mqp, C, k.shape[1]


MAX_KEY_SETS = 8


def _key_sets(who: str, sets):
    """``sets``, a sequence of 1 .. MAX_KEY_SETS (start, length, weight), as a list of (int, int, float) and as the
    (starts, lens, weights) arrays the exports take."""
    sets = [(int(s), int(n), float(w)) for s, n, w in sets]
    n = len(sets)
    if not 1 <= n <= MAX_KEY_SETS:
        raise RuntimeError(f"{who}: 1 .. {MAX_KEY_SETS} key sets, got {n}")
    return sets, ((_i64 * n)(*[s for s, _, _ in sets]), (_i64 * n)(*[m for _, m, _ in sets]),
                  (_f32 * n)(*[w for _, _, w in sets]))


def _key_rows(who: str, t, must_be: str, q: torch.Tensor, B: int, Mk: int, optional: bool = False):
    """(pointer, row length, batch stride) of fp32 per-key rows on q's device, THE statement of how they are handed over:
    (B, >= Mk) with a row per sample or (1, >= Mk) with one row for all, unit stride along the row; a batch stride of 0 is an
    expanded row.  ``must_be``: how the message opens ("bias must be").  ``optional``: None gives (None, 0, 0)."""
    if t is None and optional:
        return None, 0, 0
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != q.device or t.dim() != 2 \
            or t.shape[0] not in (1, B) or t.shape[1] < Mk or t.stride(1) != 1 \
            or (t.shape[0] == B and B > 1 and 0 < t.stride(0) < t.shape[1]):
        raise RuntimeError(f"{who}: {must_be} fp32 on q's device, (B, >= Mk) or (1, >= Mk), contiguous along its last axis")
    return t.data_ptr(), t.shape[1], (t.stride(0) if t.shape[0] == B and B > 1 else 0)


def _qk_views(who: str, q, k, heads: int, Mq: int, Mk: int, dense_single: bool):
    """The q (B, Mqp, C) / k (B, Mkp, C) views of the map calls: fp16 / bf16 on one GPU, C a multiple of heads, Mq / Mk
    inside, 16-byte aligned rows, the samples a dense stride apart -- which a single sample need not show unless
    ``dense_single``.  Returns (B, Mqp, C, Mkp, heads, Mq, Mk), the last three as ints."""
    _half_operands(who, q, k)
    if q.dim() != 3 or k.dim() != 3 or not q.is_cuda or k.device != q.device:
        raise RuntimeError(f"{who}: q must be (B, Mqp, C) and k (B, Mkp, C) on one GPU")
    B, Mqp, C = q.shape
    Mkp = k.shape[1]
    heads, Mq, Mk = int(heads), int(Mq), int(Mk)
    if k.shape[0] != B or k.shape[2] != C or heads < 1 or C % heads:
        raise RuntimeError(f"{who}: k must be (B, Mkp, C) with C a multiple of heads")
    if not (1 <= Mq <= Mqp and 1 <= Mk <= Mkp):
        raise RuntimeError(f"{who}: Mq / Mk must lie inside q / k")
    for t, name, rows in ((q, "q", Mqp), (k, "k", Mkp)):
        if t.stride(2) != 1 or t.stride(1) % 8 or t.stride(1) < C or t.data_ptr() % 16 \
                or ((dense_single or B > 1) and t.stride(0) != rows * t.stride(1)):
            raise RuntimeError(f"{who}: {name} must be 16-byte aligned rows (stride a multiple of 8), dense over the samples")
    return B, Mqp, C, Mkp, heads, Mq, Mk


@_on_device
def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, M: int, scale: float,
              share_groups: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q, k: (B, Mp, C) views with arbitrary last-dim-contiguous row stride; vt: (B, C, ldvt) = v transposed.
    Returns out (B, Mp, C) (rows >= M untouched/zero).  ``out``: a dense (B, Mp, C) tensor of q's dtype to write into (a
    sample range of a larger buffer) instead of a new one; its rows >= M are left alone."""
    if out is not None:
        _out_like_q("attention", out, q)
    B, Mp, C = q.shape
    d = C // heads
    new = _attention_out(q, k, vt, M, Mp, alloc=out is None)
    out = new if out is None else out
    ws, nb = _attention_ws(B, heads, M, M, d, q.device, q.dtype)
    _check(lib().vtm_attention(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1),
                               out.data_ptr(), C, dtype_code(q), B, heads, M, Mp, d, float(scale),
                               int(share_groups), _ptr(ws), nb, _stream()), "vtm_attention")
    return out


@_on_device
def cfg_ddim(x: Optional[torch.Tensor], eps_uncond: torch.Tensor, eps_cond: Optional[torch.Tensor], guidance: float,
             a: float, b: float, c: float, d: float, want_eps: bool = False):
    """generate.py:276-278 + 281-311 fused: returns x_next (and the guided eps when want_eps)."""
    _req(eps_uncond, "eps_uncond")
    n = eps_uncond.numel()
    # the reference's coefficients are 0-dim fp32 tensors.  torch's CPU kernels (the parity oracle) cast the
    # multipliers b, c, d to the tensor dtype before the op but divide by the ORIGINAL fp32 value of a
    # (tests/golden/ddim.npz pins this for fp16); for fp32 tensors all four are used as they are.
    b, c, d = (float(torch.tensor(v, dtype=torch.float32).to(eps_uncond.dtype)) for v in (b, c, d))
    a = float(torch.tensor(a, dtype=torch.float32))
    x_out = torch.empty_like(eps_uncond) if x is not None else None
    eps_out = torch.empty_like(eps_uncond) if (want_eps or x is None) else None
    _check(lib().vtm_cfg_ddim(_ptr(x), _ptr(eps_uncond), _ptr(eps_cond), dtype_code(eps_uncond), n, float(guidance),
                              float(a), float(b), float(c), float(d), _ptr(eps_out), _ptr(x_out), _stream()),
           "vtm_cfg_ddim")
    return (x_out, eps_out) if want_eps else (x_out if x is not None else eps_out)


PRED_EPSILON, PRED_V, PRED_SAMPLE = 0, 1, 2     # include/vidtome_hip.h VTM_PRED_*
GUIDED_STEP_THREADS = 1024                      # csrc/guided_step.hip: threads of the per-frame (rescale) workgroup


NOISE_INIT, NOISE_STEP, NOISE_LEVELS, NOISE_USER = 0, 1, 2, 16     # include/vidtome_hip.h VTM_NOISE_*


def _noise_key(who: str, key, noise=None):
    """``key`` of a keyed call, checked: None, or (seed in [0, 2^64), step in [0, 2^32), tag in [0, 2^32)) as ints; it
    stands in place of ``noise``."""
    if key is None:
        return None
    if noise is not None:
        raise RuntimeError(f"{who}: both a noise tensor and a noise key")
    try:
        seed, step, tag = (operator.index(v) for v in key)
    except (TypeError, ValueError):
        raise RuntimeError(f"{who}: key must be three integers (seed, step, tag)") from None
    if not 0 <= seed < 2 ** 64 or not 0 <= step < 2 ** 32 or not 0 <= tag < 2 ** 32:
        raise RuntimeError(f"{who}: key (seed {seed}, step {step}, tag {tag}) outside [0, 2^64) x [0, 2^32) x [0, 2^32)")
    return seed, step, tag


def guided_step_chunk(dtype: torch.dtype) -> int:
    """Elements of a 16-byte chunk, the unit csrc/guided_step.hip moves and hands to a lane (4 fp32, 8 fp16 / bf16)."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def _frame_rows(frame_ids, n_frames: int, who: str):
    """frame_ids of a guided step -> (first row, device ids or None, F).  A host sequence / CPU tensor is checked here (range,
    duplicates); an ascending run start, start + 1, ... needs no ids on the device at all: it is a row offset.  A device
    int32 tensor is taken as it is."""
    if frame_ids is None:
        return 0, None, n_frames
    if isinstance(frame_ids, torch.Tensor) and frame_ids.is_cuda:
        if frame_ids.dtype != torch.int32 or frame_ids.dim() != 1 or not frame_ids.is_contiguous():
            raise RuntimeError(f"{who}: device frame_ids must be a contiguous 1-D int32 tensor")
        return 0, frame_ids, frame_ids.numel()
    if isinstance(frame_ids, torch.Tensor):
        if frame_ids.dim() != 1 or frame_ids.dtype.is_floating_point or frame_ids.dtype == torch.bool:
            raise RuntimeError(f"{who}: frame_ids must be a 1-D integer tensor")
        frame_ids = frame_ids.tolist()
    ids = [int(i) for i in frame_ids]
    if any(i != j for i, j in zip(ids, frame_ids)):
        raise RuntimeError(f"{who}: frame_ids must be integers")
    if any(not 0 <= i < n_frames for i in ids):
        raise RuntimeError(f"{who}: frame_ids outside [0, {n_frames})")
    if len(set(ids)) != len(ids):
        raise RuntimeError(f"{who}: frame_ids holds a frame twice")
    if ids and ids == list(range(ids[0], ids[0] + len(ids))):
        return ids[0], None, len(ids)
    return 0, ids, len(ids)


def _step_operands(who: str, x, model_out, groups: int, pred_type: int, rescale: float, frame_ids, noise, noise_coef, out, want,
                   any_output: bool, check_groups, check_rescale, check_more=None, extra=()):
    """What guided_step and solver_step check and allocate alike, in the order they always did; the wrapper's own checks run
    in between: ``check_groups()`` after the operand types, ``check_rescale(E)`` once the shapes fit, ``check_more()`` after
    the noise.  ``noise_coef``: the name of the non-zero coefficient that needs ``noise``, or None; ``want`` = (want_x,
    want_eps, want_x0); ``extra``: further (tensor or None, name) pairs that must live on x's device.  Returns
    (F, E, device frame ids or None, out, eps, x0, the chunk's first element in a whole-video tensor)."""
    for t, name in ((x, "x"), (model_out, "model_out")):
        if not isinstance(t, torch.Tensor) or t.dim() < 2 or t.dtype not in _DT:
            raise RuntimeError(f"{who}: {name} must be a (frames, ...) fp16 / bf16 / fp32 tensor")
    if pred_type not in (PRED_EPSILON, PRED_V, PRED_SAMPLE):
        raise RuntimeError(f"{who}: unknown pred_type {pred_type}")
    check_groups()
    if not rescale >= 0.0:
        raise RuntimeError(f"{who}: rescale = {rescale} is negative or NaN")
    first, ids, F = _frame_rows(frame_ids, x.shape[0], who)
    E = math.prod(x.shape[1:])
    if model_out.shape[0] != groups * F or math.prod(model_out.shape[1:]) != E:
        raise RuntimeError(f"{who}: model_out {tuple(model_out.shape)} is not ({groups} groups * {F} frames, {E} elements)")
    if model_out.dtype != x.dtype:
        raise RuntimeError(f"{who}: dtype mismatch: x {x.dtype}, model_out {model_out.dtype}")
    check_rescale(E)
    if noise_coef and noise is None:
        raise RuntimeError(f"{who}: {noise_coef} != 0 needs noise")
    if noise is not None and (not isinstance(noise, torch.Tensor) or noise.dtype != x.dtype or noise.numel() != F * E
                              or noise.shape[0] != F):
        raise RuntimeError(f"{who}: noise must be a ({F}, ...) {x.dtype} tensor of the chunk's {F * E} elements")
    if check_more:
        check_more()
    if not any_output:
        raise RuntimeError(f"{who}: no output asked for")
    if out is not None and (not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype
                            or out.device != x.device):
        raise RuntimeError(f"{who}: out must be a tensor like x (it may be x)")
    if E < 1 and F:
        raise RuntimeError(f"{who}: empty frames")
    _req(x, "x"), _req(model_out, "model_out")
    for t, name in ((noise, "noise"), (out, "out"), *extra, (ids if isinstance(ids, torch.Tensor) else None, "frame_ids")):
        if t is not None and _req(t, name).device != x.device:
            raise RuntimeError(f"{who}: {name} lives on {t.device}, x on {x.device}")
    if model_out.device != x.device:
        raise RuntimeError(f"{who}: model_out lives on {model_out.device}, x on {x.device}")
    if isinstance(ids, list):
        ids = torch.tensor(ids, dtype=torch.int32, device=x.device)
    want_x, want_eps, want_x0 = want
    if want_x and out is None:
        out = torch.empty_like(x) if (frame_ids is None) else x
    local = (F,) + tuple(model_out.shape[1:])
    eps = torch.empty(local, dtype=x.dtype, device=x.device) if want_eps else None
    x0 = torch.empty(local, dtype=x.dtype, device=x.device) if want_x0 else None
    return F, E, ids, out, eps, x0, first * E


@_on_device
def guided_step(x: torch.Tensor, model_out: torch.Tensor, sqrt_alpha: float, sqrt_beta: float, c_x0: float, c_eps: float,
                sigma: float = 0.0, *, groups: int = 2, g_uncond: Optional[int] = None, g_cond: Optional[int] = None,
                frame_ids=None, pred_type: int = PRED_EPSILON, guidance: float = 7.5, rescale: float = 0.0,
                noise: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, want_x: bool = True,
                want_eps: bool = False, want_x0: bool = False, key=None):
    """One chunk's guided DDIM step (vtm_guided_step, include/vidtome_hip.h): ``x`` (n_frames, ...) the whole-video latents,
    ``model_out`` (groups * F, ...) the UNet output of the chunk, group-major; the chunk's frame f is row ``frame_ids[f]`` of x
    (a host sequence / CPU tensor, checked and uploaded unless it is an ascending run; or a device int32 tensor, taken as it
    is; None: the chunk is the whole video).  ``g_uncond`` / ``g_cond`` default to the last two groups (one group: no
    guidance, g_cond = -1).  ``out`` receives x' in the chunk's rows and may be x; None allocates a new tensor when the chunk
    is the whole video and otherwise means x (in place: a new tensor would have rows that nobody wrote).  Returns
    (out or None, eps or None, x0 or None) -- eps / x0 chunk-local (F, ...), allocated when asked for.  ``key`` = (seed, step,
    tag) in place of ``noise``: the frame-keyed noise of those frames, drawn inside the launch (vtm_guided_step_keyed)."""
    who = "guided_step"
    key = _noise_key(who, key, noise)
    groups = int(groups)
    if g_uncond is None:
        g_uncond = max(groups - 2, 0)
    if g_cond is None:
        g_cond = groups - 1 if groups >= 2 else -1
    g_uncond, g_cond, pred_type, sigma, rescale = int(g_uncond), int(g_cond), int(pred_type), float(sigma), float(rescale)

    def check_groups():
        if groups < 1 or not 0 <= g_uncond < groups or not -1 <= g_cond < groups:
            raise RuntimeError(f"{who}: groups = {groups}, g_uncond = {g_uncond}, g_cond = {g_cond}: a group index outside "
                               "[0, groups)")
        if g_uncond == g_cond:
            raise RuntimeError(f"{who}: g_uncond == g_cond == {g_cond}")

    def check_rescale(E):
        if rescale > 0.0 and (g_cond < 0 or E < 2):
            raise RuntimeError(f"{who}: rescale > 0 needs a conditional group and frames of at least 2 elements")

    F, E, ids, out, eps, x0, skip = _step_operands(
        who, x, model_out, groups, pred_type, rescale, frame_ids, noise, "sigma" if sigma != 0.0 and key is None else None, out,
        (want_x, want_eps, want_x0), want_x or want_eps or want_x0, check_groups, check_rescale)
    if F == 0:
        return (out if want_x else None), eps, x0
    frame0 = skip // E
    skip *= x.element_size()
    if key is not None:
        _check(lib().vtm_guided_step_keyed(x.data_ptr() + skip, model_out.data_ptr(), *key, frame0, dtype_code(x), F, E, groups,
                                           g_uncond, g_cond, _ptr(ids), pred_type, float(guidance), rescale, float(sqrt_alpha),
                                           float(sqrt_beta), float(c_x0), float(c_eps), sigma,
                                           out.data_ptr() + skip if want_x else None, _ptr(eps), _ptr(x0), _stream()),
               "vtm_guided_step_keyed")
        return (out if want_x else None), eps, x0
    _check(lib().vtm_guided_step(x.data_ptr() + skip, model_out.data_ptr(), _ptr(noise if sigma != 0.0 else None),
                                 dtype_code(x), F, E, groups, g_uncond, g_cond, _ptr(ids), pred_type, float(guidance),
                                 rescale, float(sqrt_alpha), float(sqrt_beta), float(c_x0), float(c_eps), sigma,
                                 out.data_ptr() + skip if want_x else None, _ptr(eps), _ptr(x0), _stream()),
           "vtm_guided_step")
    return (out if want_x else None), eps, x0


SOLVER_STEP_THREADS = 1024                      # csrc/solver_step.hip: threads of the per-frame (rescale) workgroup
SOLVER_MAX_GROUPS = 8                           # include/vidtome_hip.h VTM_SOLVER_MAX_GROUPS


def _solver_checks(who: str, x, weights, pred_type, g_ref, rescale: float, fp32_like_x):
    """What solver_step and invert_step check about the weights, the rescale reference and their whole-video fp32 operands:
    -> (weights, groups, pred_type, g_ref, check_groups, check_rescale, check_history), the three checks as ``_step_operands``
    calls them.  ``fp32_like_x``: (tensor or None, name, the coefficient that needs it) triples."""
    weights = [float(v) for v in weights]
    groups, pred_type = len(weights), int(pred_type)
    g_ref = groups - 1 if g_ref is None else int(g_ref)

    def check_groups():
        if not 1 <= groups <= SOLVER_MAX_GROUPS or not all(math.isfinite(v) for v in weights):
            raise RuntimeError(f"{who}: {groups} weights {weights}: 1 .. {SOLVER_MAX_GROUPS} finite numbers, one per group")

    def check_rescale(E):
        if rescale > 0.0 and (not 0 <= g_ref < groups or _f32_round(weights[g_ref]) == 0.0 or E < 2):
            raise RuntimeError(f"{who}: rescale > 0 needs g_ref = {g_ref} inside [0, {groups}) with a non-zero weight, and "
                               "frames of at least 2 elements")

    def check_history():
        for t, name, c in fp32_like_x:
            if t is None and c != 0.0:
                raise RuntimeError(f"{who}: c_{name} != 0 needs {name}")
            if t is not None and (not isinstance(t, torch.Tensor) or t.shape != x.shape or t.dtype != torch.float32
                                  or t.device != x.device):
                raise RuntimeError(f"{who}: {name} must be an fp32 tensor shaped like x, on its device")

    return weights, groups, pred_type, g_ref, check_groups, check_rescale, check_history


@_on_device
def solver_step(x: torch.Tensor, model_out: torch.Tensor, weights, sqrt_alpha: float, sqrt_beta: float, c_x: float, c_x0: float,
                c_h1: float = 0.0, c_h2: float = 0.0, c_noise: float = 0.0, *, h1: Optional[torch.Tensor] = None,
                h2: Optional[torch.Tensor] = None, h_out: Optional[torch.Tensor] = None, g_ref: Optional[int] = None,
                frame_ids=None, pred_type: int = PRED_EPSILON, rescale: float = 0.0, noise: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, want_x: bool = True, want_eps: bool = False, want_x0: bool = False,
                key=None):
    """One chunk's step of a multistep solver (vtm_solver_step, include/vidtome_hip.h): ``x``, ``model_out``, ``frame_ids``,
    ``noise`` or ``key`` (vtm_solver_step_keyed), ``out`` and the result (out or None, eps or None, x0 or None) as in
    ``guided_step``.  ``weights``: one host
    number per group of model_out (their count is the number of groups; a group of weight 0 is never read); ``g_ref``: the
    group whose per-frame std ``rescale`` restores (default: the last).  ``h1`` / ``h2``: whole-video fp32 tensors shaped like
    x with the clean-sample predictions of the two previous steps, needed where ``c_h1`` / ``c_h2`` is not 0; ``h_out``: where
    this step's goes (it may be h1 or h2)."""
    who = "solver_step"
    key = _noise_key(who, key, noise)
    c_x, c_x0, c_h1, c_h2, c_noise, rescale = (float(v) for v in (c_x, c_x0, c_h1, c_h2, c_noise, rescale))
    weights, groups, pred_type, g_ref, check_groups, check_rescale, check_history = _solver_checks(
        who, x, weights, pred_type, g_ref, rescale, ((h1, "h1", c_h1), (h2, "h2", c_h2), (h_out, "h_out", 0.0)))

    F, E, ids, out, eps, x0, skip = _step_operands(
        who, x, model_out, groups, pred_type, rescale, frame_ids, noise, "c_noise" if c_noise != 0.0 and key is None else None, out,
        (want_x, want_eps, want_x0), want_x or want_eps or want_x0 or h_out is not None, check_groups, check_rescale,
        check_history, ((h1, "h1"), (h2, "h2"), (h_out, "h_out")))
    if F == 0:
        return (out if want_x else None), eps, x0

    def hist(t, used=True):
        return t.data_ptr() + skip * 4 if (t is not None and used) else None
    skip_x = skip * x.element_size()
    if key is not None:
        _check(lib().vtm_solver_step_keyed(x.data_ptr() + skip_x, model_out.data_ptr(), *key, skip // E, hist(h1, c_h1 != 0.0),
                                           hist(h2, c_h2 != 0.0), dtype_code(x), F, E, groups, (_f32 * groups)(*weights), g_ref,
                                           _ptr(ids), pred_type, rescale, float(sqrt_alpha), float(sqrt_beta), c_x, c_x0, c_h1,
                                           c_h2, c_noise, out.data_ptr() + skip_x if want_x else None, hist(h_out), _ptr(eps),
                                           _ptr(x0), _stream()), "vtm_solver_step_keyed")
        return (out if want_x else None), eps, x0
    _check(lib().vtm_solver_step(x.data_ptr() + skip_x, model_out.data_ptr(), _ptr(noise if c_noise != 0.0 else None),
                                 hist(h1, c_h1 != 0.0), hist(h2, c_h2 != 0.0), dtype_code(x), F, E, groups,
                                 (_f32 * groups)(*weights), g_ref, _ptr(ids), pred_type, rescale, float(sqrt_alpha),
                                 float(sqrt_beta), c_x, c_x0, c_h1, c_h2, c_noise, out.data_ptr() + skip_x if want_x else None,
                                 hist(h_out), _ptr(eps), _ptr(x0), _stream()), "vtm_solver_step")
    return (out if want_x else None), eps, x0


@_on_device
def invert_step(x: torch.Tensor, model_out: torch.Tensor, weights, sqrt_alpha: float, sqrt_beta: float, c_x: float, c_x0: float,
                c_h1: float = 0.0, c_h2: float = 0.0, c_noise: float = 0.0, *, target: Optional[torch.Tensor] = None,
                z_out: Optional[torch.Tensor] = None, h1: Optional[torch.Tensor] = None, h2: Optional[torch.Tensor] = None,
                h_out: Optional[torch.Tensor] = None, g_ref: Optional[int] = None, frame_ids=None,
                pred_type: int = PRED_EPSILON, rescale: float = 0.0, want_eps: bool = False, want_x0: bool = False):
    """One chunk's step of edit-friendly inversion (vtm_invert_step, include/vidtome_hip.h), the inverse of ``solver_step``:
    ``x`` the current level and ``target`` the next one, whole-video tensors of one shape and dtype; ``z_out`` like them
    receives the step's noise in the chunk's rows, and ``target`` is corrected IN PLACE there, to exactly what ``solver_step``
    computes from the same operands with ``noise = z_out[rows]``.  With ``c_noise == 0`` z_out's rows become +0 and target
    (it may be None) is left alone.  ``model_out``, ``weights``, ``g_ref``, ``h1`` / ``h2`` / ``h_out``, ``frame_ids``,
    ``pred_type`` and ``rescale`` as in ``solver_step``.  Returns (eps or None, x0 or None), chunk-local."""
    who = "invert_step"
    c_x, c_x0, c_h1, c_h2, c_noise, rescale = (float(v) for v in (c_x, c_x0, c_h1, c_h2, c_noise, rescale))
    weights, groups, pred_type, g_ref, check_groups, check_rescale, check_history = _solver_checks(
        who, x, weights, pred_type, g_ref, rescale, ((h1, "h1", c_h1), (h2, "h2", c_h2), (h_out, "h_out", 0.0)))

    def check_more():
        check_history()
        if z_out is None or (target is None and c_noise != 0.0):
            raise RuntimeError(f"{who}: z_out is required, and c_noise != 0 needs target")
        for t, name in ((target, "target"), (z_out, "z_out")):
            if t is not None and (not isinstance(t, torch.Tensor) or t.shape != x.shape or t.dtype != x.dtype
                                  or t.device != x.device):
                raise RuntimeError(f"{who}: {name} must be a tensor like x, on its device")
        if len({t.data_ptr() for t in (x, target, z_out) if t is not None}) != 2 + (target is not None):
            raise RuntimeError(f"{who}: x, target and z_out must be three buffers")

    F, E, ids, _, eps, x0, skip = _step_operands(
        who, x, model_out, groups, pred_type, rescale, frame_ids, None, None, None, (False, want_eps, want_x0), True,
        check_groups, check_rescale, check_more, ((h1, "h1"), (h2, "h2"), (h_out, "h_out"), (target, "target"), (z_out, "z_out")))
    if F == 0:
        return eps, x0

    def row(t, size, used=True):
        return t.data_ptr() + skip * size if (t is not None and used) else None
    el = x.element_size()
    _check(lib().vtm_invert_step(row(x, el), model_out.data_ptr(), row(h1, 4, c_h1 != 0.0), row(h2, 4, c_h2 != 0.0),
                                 dtype_code(x), F, E, groups, (_f32 * groups)(*weights), g_ref, _ptr(ids), pred_type, rescale,
                                 float(sqrt_alpha), float(sqrt_beta), c_x, c_x0, c_h1, c_h2, c_noise,
                                 row(target, el, c_noise != 0.0), row(z_out, el), row(h_out, 4), _ptr(eps), _ptr(x0), _stream()),
           "vtm_invert_step")
    return eps, x0


@_on_device
def noise_levels(x0: torch.Tensor, levels: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """levels[k] = coef[k, 0] * x0 + coef[k, 1] * levels[k] in place, all levels in one launch (vtm_noise_levels): ``levels``
    (n, *x0.shape) holds independent N(0, 1) draws in x0's dtype, ``coef`` is a device fp32 (n, 2) table of (sqrt_alpha,
    sqrt_beta).  Returns levels."""
    who = "noise_levels"
    for t, name in ((x0, "x0"), (levels, "levels"), (coef, "coef")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{who}: {name} must be a tensor")
    if x0.dtype not in _DT or levels.dtype != x0.dtype:
        raise RuntimeError(f"{who}: x0 and levels must share one of fp16 / bf16 / fp32, not {x0.dtype} and {levels.dtype}")
    if levels.dim() != x0.dim() + 1 or tuple(levels.shape[1:]) != tuple(x0.shape) or x0.numel() < 1:
        raise RuntimeError(f"{who}: levels {tuple(levels.shape)} is not (n, *x0.shape) for x0 {tuple(x0.shape)}")
    n = levels.shape[0]
    if coef.dtype != torch.float32 or tuple(coef.shape) != (n, 2):
        raise RuntimeError(f"{who}: coef must be an fp32 ({n}, 2) tensor of (sqrt_alpha, sqrt_beta)")
    _req(x0, "x0"), _req(levels, "levels"), _req(coef, "coef")
    if levels.device != x0.device or coef.device != x0.device:
        raise RuntimeError(f"{who}: levels lives on {levels.device}, coef on {coef.device}, x0 on {x0.device}")
    if n:
        _check(lib().vtm_noise_levels(x0.data_ptr(), levels.data_ptr(), coef.data_ptr(), dtype_code(x0), n, x0.numel(),
                                      _stream()), "vtm_noise_levels")
    return levels


@_on_device
def frame_noise(out: torch.Tensor, seed: int, step0: int, tag: int, frame_ids=None, n_frames: Optional[int] = None
                ) -> torch.Tensor:
    """Frame-keyed N(0, 1) noise (vtm_frame_noise, include/vidtome_hip.h "Frame-keyed noise") into ``out`` (S, F, ...),
    contiguous fp16 / bf16 / fp32 on the GPU: out[s, f] is the noise of whole-video frame ``frame_ids[f]`` (a host sequence,
    checked against ``n_frames`` when that is given; or a device int32 tensor, taken as it is; None: frame f, and ``n_frames``
    when given must be F) at step
    ``step0 + s``.  One launch.  Returns out."""
    who = "frame_noise"
    if not isinstance(out, torch.Tensor) or out.dim() < 3 or out.dtype not in _DT:
        raise RuntimeError(f"{who}: out must be a (steps, frames, ...) fp16 / bf16 / fp32 tensor")
    seed, step0, tag = _noise_key(who, (seed, step0, tag))
    S, F = out.shape[0], out.shape[1]
    E = math.prod(out.shape[2:])
    if frame_ids is None:
        if n_frames is not None and int(n_frames) != F:
            raise RuntimeError(f"{who}: n_frames = {n_frames} for out's {F} frames (without frame_ids they are frames 0 .. F - 1)")
        first, ids = 0, None
    else:
        first, ids, n = _frame_rows(frame_ids, 2 ** 31 if n_frames is None else int(n_frames), who)
        if n != F:
            raise RuntimeError(f"{who}: {n} frame_ids for out's {F} frames")
    if E < 1 and S and F:
        raise RuntimeError(f"{who}: empty frames")
    _req(out, "out")
    if isinstance(ids, torch.Tensor) and _req(ids, "frame_ids").device != out.device:
        raise RuntimeError(f"{who}: frame_ids lives on {ids.device}, out on {out.device}")
    if isinstance(ids, list):
        ids = torch.tensor(ids, dtype=torch.int32, device=out.device)
    if S and F:
        _check(lib().vtm_frame_noise(out.data_ptr(), dtype_code(out), S, F, E, _ptr(ids), first, seed, step0, tag, _stream()),
               "vtm_frame_noise")
    return out


@_on_device
def philox_bits(counters: torch.Tensor, seed: int) -> torch.Tensor:
    """Philox4x32-10 of every row of ``counters`` (n, 4) under the key of ``seed`` (vtm_philox_bits): a new (n, 4) tensor.
    Both are device int32 tensors holding the uint32 bit patterns (torch's uint32 support is partial)."""
    who = "philox_bits"
    if not isinstance(counters, torch.Tensor) or counters.dtype != torch.int32 or counters.dim() != 2 or counters.shape[1] != 4:
        raise RuntimeError(f"{who}: counters must be an (n, 4) int32 tensor of uint32 bit patterns")
    seed = _noise_key(who, (seed, 0, 0))[0]
    _req(counters, "counters")
    out = torch.empty_like(counters)
    if counters.shape[0]:
        _check(lib().vtm_philox_bits(counters.data_ptr(), counters.shape[0], seed, out.data_ptr(), _stream()), "vtm_philox_bits")
    return out


@_on_device
def layernorm(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    """torch.nn.LayerNorm over the last axis (patch.py:139-146 `self.norm1(hidden_states)`)."""
    _req(x, "x")
    C = x.shape[-1]
    xc = x.contiguous()
    for name, p in (("weight", weight), ("bias", bias)):
        if p is not None and (p.dtype != x.dtype or p.numel() != C or p.device != x.device):
            raise RuntimeError(f"vidtome_amd: layernorm {name} must be a ({C},) {x.dtype} tensor on {x.device}")
    out = torch.empty_like(xc)
    _check(lib().vtm_layernorm(_ptr(xc), _ptr(weight.contiguous() if weight is not None else None),
                               _ptr(bias.contiguous() if bias is not None else None), dtype_code(xc),
                               xc.numel() // C, C, float(eps), _ptr(out), _stream()), "vtm_layernorm")
    return out


@_on_device
def attention_kv(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, Mq: int, Mk: int, scale: float,
                 use_workspace: bool = True, q_count: Optional[torch.Tensor] = None,
                 k_fold: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, share_groups: int = 1,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Cross-attention core (patch.py:178-183): q (B, Mqp, C), k (B, Mkp, C) views contiguous along the last axis,
    vt (B, C, ldvt >= Mk) = v transposed.  Returns (B, Mqp, C).  ``q_count`` (B,) int32 on the device: only the first
    q_count[b] query rows of sample b are meaningful (compact_queries); the other rows of the result are undefined.
    ``k_fold`` = (k_count (B,) int32, k_bias (B, >= Mk) uint32 pairs) from fold_keys: k / vt hold a duplicate-free key
    list, only the first k_count[b] entries are keys, each standing for 2^bias identical ones (head dims 8 and 40).
    ``share_groups`` > 1: the probabilities of the first B / share_groups samples serve every group (pnp_utils.py:57-67);
    with ``q_count`` the caller vouches that every sample of a group has the same live rows (align_batch) -- no key folding.
    ``out``: a dense (B, Mqp, C) tensor of q's dtype to write into (a sample range of a larger buffer) instead of a new one."""
    if out is not None:
        _out_like_q("attention_kv", out, q)
    if share_groups != 1 and k_fold is not None:
        raise RuntimeError("attention_kv: shared probabilities do not go with folded keys")
    if k_fold is not None and q.dtype == torch.float32:
        raise RuntimeError("attention_kv: fp32 keys are never folded (k_fold takes fp16 / bf16 operands)")
    B, Mqp, C = q.shape
    Mkp = k.shape[1]
    d = C // heads
    new = _attention_out(q, k, vt, Mq, Mkp, alloc=out is None)
    out = new if out is None else out
    ws, nb = _attention_ws(B, heads, Mq, Mk, d, q.device, q.dtype) if use_workspace else (None, 0)
    if q_count is not None and (q_count.dtype != torch.int32 or q_count.numel() != B or not q_count.is_cuda):
        raise RuntimeError("attention_kv: q_count must be a (B,) int32 device tensor")
    if q_count is not None and use_workspace and SPLIT_ALL_BOUNDED:
        nb2 = int(lib().vtm_attention_kv_bounded_ws_bytes_dtype(_DT[q.dtype], B, heads, Mq, Mk, d))
        if nb2 > nb:
            ws, nb = _workspace("attention", nb2, q.device), nb2
    if share_groups != 1 and q_count is not None:
        _check(lib().vtm_attention_kv_shared_bounded(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(),
                                                     vt.stride(1), out.data_ptr(), C, dtype_code(q), B, heads, Mq, Mqp, Mk, Mkp,
                                                     d, float(scale), int(share_groups), _ptr(q_count), _ptr(ws), nb, _stream()),
               "vtm_attention_kv_shared_bounded")
        return out
    if k_fold is not None:
        k_count, k_bias = k_fold
        if k_count.dtype != torch.int32 or k_count.numel() != B or k_bias.dtype != torch.int32 or k_bias.dim() != 2 \
                or k_bias.shape[0] != B or k_bias.shape[1] < Mk or not k_bias.is_contiguous():
            raise RuntimeError("attention_kv: k_fold must be ((B,) int32 counts, (B, >= Mk) int32 bias words)")
        _check(lib().vtm_attention_kv_folded(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1),
                                             out.data_ptr(), C, dtype_code(q), B, heads, Mq, Mqp, Mk, Mkp, d, float(scale),
                                             _ptr(q_count), _ptr(k_count), _ptr(k_bias), k_bias.shape[1], _ptr(ws), nb,
                                             _stream()), "vtm_attention_kv_folded")
        return out
    if q_count is not None:
        _check(lib().vtm_attention_kv_bounded(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(),
                                              vt.stride(1), out.data_ptr(), C, dtype_code(q), B, heads, Mq, Mqp, Mk, Mkp,
                                              d, float(scale), _ptr(q_count), _ptr(ws), nb, _stream()),
               "vtm_attention_kv_bounded")
        return out
    _check(lib().vtm_attention_kv(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1),
                                  out.data_ptr(), C, dtype_code(q), B, heads, Mq, Mqp, Mk, Mkp, d, float(scale),
                                  int(share_groups), _ptr(ws), nb, _stream()), "vtm_attention_kv")
    return out


@_on_device
def attention_kv_range(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, Mq: int, start: int, Mk: int,
                       scale: float) -> torch.Tensor:
    """attention_kv over the key range [start, start + Mk) of k (B, Mkp, C) / vt (B, C, ldvt), start a multiple of 8: the
    same vtm_attention_kv launch on the buffers where they are (pointers moved to the range, the buffers' own strides).
    start == 0 IS attention_kv(q, k, vt, heads, Mq, Mk, scale)."""
    start, Mk = int(start), int(Mk)
    B, Mqp, C = q.shape
    Mkp = k.shape[1]
    if start % 8 or start < 0 or Mk < 1 or start + Mk > Mkp or start + Mk > vt.shape[2]:
        raise RuntimeError("attention_kv_range: the range must start on a multiple of 8 and lie inside k and vt")
    if start == 0:
        return attention_kv(q, k, vt, heads, Mq, Mk, scale)
    d = C // heads
    out = _attention_out(q, k, vt, Mq, Mkp)
    ws, nb = _attention_ws(B, heads, Mq, Mk, d, q.device, q.dtype)
    es = k.element_size()
    # (sample b's keys start at k + (b * Mkp + start) * ldk: the row count Mkp stays the sample stride)
    _check(lib().vtm_attention_kv(q.data_ptr(), q.stride(1), k.data_ptr() + start * k.stride(1) * es, k.stride(1),
                                  vt.data_ptr() + start * es, vt.stride(1), out.data_ptr(), C, dtype_code(q), B, heads, Mq, Mqp,
                                  Mk, Mkp, d, float(scale), 1, _ptr(ws), nb, _stream()), "vtm_attention_kv")
    return out


@_on_device
def attention_kv_sets(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, Mq: int, sets, scale: float
                      ) -> torch.Tensor:
    """Cross-attention over several key sets, one softmax per set (vtm_attention_kv_sets): q (B, Mqp, C), k (B, Mkp, C)
    views contiguous along the last axis, vt (B, C, ldvt) = v transposed, as for attention_kv.  ``sets`` is a sequence of
    (start, length, weight): set s is the key range [start, start + length) of k / vt, start a multiple of 8; the result
    is sum_s weight_s * softmax(q K_s^T * scale) V_s, (B, Mqp, C).  fp16 / bf16 operands only.  One set of weight 1 IS the
    plain core and goes to attention_kv (the same launch and bits as a block without the extra sets)."""
    who = "attention_kv_sets"
    sets, arrays = _key_sets(who, sets)
    _half_operands(who, q, k, vt, _MODULE_PATH)
    _attention_out(q, k, vt, Mq, k.shape[1], alloc=False)
    B, Mqp, C, Mkp = _kv_shapes(who, q, k, vt)
    if len(sets) == 1 and sets[0][2] == 1.0:
        return attention_kv_range(q, k, vt, heads, Mq, sets[0][0], sets[0][1], scale)
    out = _attention_out(q, k, vt, Mq, Mkp)
    _check(lib().vtm_attention_kv_sets(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1),
                                       out.data_ptr(), C, dtype_code(q), B, heads, Mq, Mqp, Mkp, C // heads, float(scale),
                                       len(sets), *arrays, _stream()), "vtm_attention_kv_sets")
    return out


@_on_device
def attention_kv_sets_masked(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, Mq: int, sets, scale: float,
                             set_mask, mask: Optional[torch.Tensor]) -> torch.Tensor:
    """attention_kv_sets with a weight per query on chosen sets (vtm_attention_kv_sets_masked): ``set_mask[s]`` is -1 (set s
    is weighted by its scalar alone) or a row of ``mask``, fp32 on q's device, (R, ld) -- one table for every sample, what
    Diffusers' ``ip_adapter_masks`` give -- or (B, R, ld) with a table per sample; ld >= Mq, the weights are shared by the
    heads.  The result is sum_s weight_s * mask[set_mask[s]][query] * softmax(q K_s^T * scale) V_s, the masked term weighted
    in fp32.  With every ``set_mask[s] == -1`` this IS attention_kv_sets(q, k, vt, heads, Mq, sets, scale)."""
    who = "attention_kv_sets_masked"
    sets = list(sets)
    rows = [int(r) for r in set_mask]
    if len(rows) != len(sets):
        raise RuntimeError(f"{who}: {len(sets)} sets but {len(rows)} mask rows")
    if all(r == -1 for r in rows):
        return attention_kv_sets(q, k, vt, heads, Mq, sets, scale)
    sets, arrays = _key_sets(who, sets)
    _half_operands(who, q, k, vt)
    B, Mqp, C, Mkp = _kv_shapes(who, q, k, vt)
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.float32 or mask.device != q.device \
            or mask.dim() not in (2, 3) or not mask.is_contiguous() or mask.shape[-1] < Mq \
            or (mask.dim() == 3 and mask.shape[0] != B):
        raise RuntimeError(f"{who}: mask must be contiguous fp32 on q's device, (R, >= Mq) or (B, R, >= Mq)")
    R, ld = mask.shape[-2], mask.shape[-1]
    if not all(-1 <= r < R for r in rows):
        raise RuntimeError(f"{who}: mask rows {rows} do not lie in the table of {R} rows")
    out = _attention_out(q, k, vt, Mq, Mkp)
    n = len(sets)
    _check(lib().vtm_attention_kv_sets_masked(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(),
                                              vt.stride(1), out.data_ptr(), C, dtype_code(q), B, heads, Mq, Mqp, Mkp,
                                              C // heads, float(scale), n, *arrays, (_int * n)(*rows), mask.data_ptr(), ld,
                                              R * ld if mask.dim() == 3 else 0, _stream()), "vtm_attention_kv_sets_masked")
    return out


@_on_device
def attention_kv_sets_src(q: torch.Tensor, q_src: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, Mq: int, sets,
                          scale: float, set_src, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attention_kv_sets with a second query operand (vtm_attention_kv_sets_src): set s takes its probabilities from
    ``q_src`` (B, Mqp_src >= Mq, C) where ``set_src[s]`` is 1 and from ``q`` where it is 0; k, vt and the result belong to
    q's samples.  q_src is a view like q (contiguous along the last axis, dense batch stride, 16-byte aligned rows) and may
    be another sample range of q's buffer.  ``out``: a dense (B, Mqp, C) tensor to write into (rows >= Mq stay as they are)
    instead of a new one.  With every ``set_src[s] == 0`` this IS attention_kv_sets' launch (the library sends it to the
    same kernel)."""
    who = "attention_kv_sets_src"
    sets = list(sets)
    src = [int(s) for s in set_src]
    if len(src) != len(sets):
        raise RuntimeError(f"{who}: {len(sets)} sets but {len(src)} set_src entries")
    sets, arrays = _key_sets(who, sets)
    if any(s not in (0, 1) for s in src):
        raise RuntimeError(f"{who}: set_src entries are 0 (q) or 1 (q_src), got {src}")
    _half_operands(who, q, k, vt)
    _attention_out(q, k, vt, Mq, k.shape[1], alloc=False)
    B, Mqp, C, Mkp = _kv_shapes(who, q, k, vt)
    if not isinstance(q_src, torch.Tensor) or q_src.dtype != q.dtype or q_src.device != q.device or q_src.dim() != 3 \
            or q_src.shape[0] != B or q_src.shape[2] != C or q_src.shape[1] < Mq or q_src.stride(2) != 1 \
            or q_src.stride(1) % 8 or q_src.stride(0) != q_src.shape[1] * q_src.stride(1) or q_src.data_ptr() % 16:
        raise RuntimeError(f"{who}: q_src must be (B, >= Mq, C) of q's dtype on q's device, 16-byte aligned rows (stride a "
                           "multiple of 8), dense over the samples")
    if out is None:
        out = _attention_out(q, k, vt, Mq, Mkp)
    else:
        _out_like_q(who, out, q)
    n = len(sets)
    _check(lib().vtm_attention_kv_sets_src(q.data_ptr(), q.stride(1), q_src.data_ptr(), q_src.stride(1), q_src.shape[1],
                                           k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1), out.data_ptr(), C,
                                           dtype_code(q), B, heads, Mq, Mqp, Mkp, C // heads, float(scale), n, *arrays,
                                           (_int * n)(*src), _stream()), "vtm_attention_kv_sets_src")
    return out


CROSS_EDIT_MAX_KEYS = 256   # what vtm_cross_edit_values takes (csrc/cross_edit.hip): vtm_attention_probs' key limit


@_on_device
def cross_edit_values(vt: torch.Tensor, v_start: int, K: int, mapper: torch.Tensor, src_w: torch.Tensor, own_w: torch.Tensor,
                      start_src: int = 0, start_own: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The value operand of an edited cross-attention call (vtm_cross_edit_values): vt (B, C, ldvt) = v transposed, fp16 /
    bf16, whose columns [v_start, v_start + K) are the keys; ``mapper`` (K, K), ``src_w`` (K,), ``own_w`` (K,) contiguous
    fp32 on vt's device.  Writes (mapper diag(src_w) V)^T to columns [start_src, start_src + K) and (diag(own_w) V)^T to
    [start_own, start_own + K) of ``out`` (B, C, ldvt_out) and returns it; a new ``out`` has start_own + K rounded up to 8
    columns and zeros outside the two ranges.  start_own defaults to start_src + K rounded up to 8."""
    v_start, K, start_src = int(v_start), int(K), int(start_src)
    start_own = start_src + (K + 7) // 8 * 8 if start_own is None else int(start_own)
    if not isinstance(vt, torch.Tensor) or vt.dtype not in (torch.float16, torch.bfloat16) or vt.dim() != 3:
        raise RuntimeError("cross_edit_values: vt must be a (B, C, ldvt) fp16 / bf16 tensor")
    _req(vt, "vt")
    if not 1 <= K <= CROSS_EDIT_MAX_KEYS:
        raise RuntimeError(f"cross_edit_values: K = {K}, 1 .. {CROSS_EDIT_MAX_KEYS} keys are taken")
    for t, name, shape in ((mapper, "mapper", (K, K)), (src_w, "src_w", (K,)), (own_w, "own_w", (K,))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != vt.device or tuple(t.shape) != shape \
                or not t.is_contiguous():
            raise RuntimeError(f"cross_edit_values: {name} must be a contiguous fp32 {shape} tensor on vt's device")
    B, C, ldvt = vt.shape
    if out is None:
        out = torch.zeros((B, C, max(start_src, start_own) + (K + 7) // 8 * 8), dtype=vt.dtype, device=vt.device)
    elif out.dim() != 3 or out.shape[:2] != vt.shape[:2] or out.dtype != vt.dtype or out.device != vt.device \
            or not out.is_contiguous():
        raise RuntimeError("cross_edit_values: out must be a contiguous (B, C, ldvt_out) tensor of vt's dtype and device")
    _check(lib().vtm_cross_edit_values(vt.data_ptr(), ldvt, v_start, dtype_code(vt), B, C, K, mapper.data_ptr(),
                                       src_w.data_ptr(), own_w.data_ptr(), out.data_ptr(), out.shape[2], start_src, start_own,
                                       _stream()), "vtm_cross_edit_values")
    return out


@_on_device
def attention_kv_bias(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, Mq: int, Mk: int, scale: float,
                      bias: torch.Tensor) -> torch.Tensor:
    """attention_kv with one additive fp32 term per key on the scores (vtm_attention_kv_bias): q (B, Mqp, C), k (B, Mkp, C)
    views contiguous along the last axis, vt (B, C, ldvt >= Mk) = v transposed, Mkp a multiple of 8, as for attention_kv.
    ``bias`` is fp32 on q's device, (B, Mk') with a row per sample or (1, Mk') with one row for all, Mk' >= Mk, contiguous
    along the last axis; the values are shared by the heads and the queries and are finite or -inf (-inf: probability exactly
    0).  The result is softmax(q K^T * scale + bias) V, (B, Mqp, C).  fp16 / bf16 operands only."""
    who = "attention_kv_bias"
    _half_operands(who, q, k, vt, _MODULE_PATH)
    B, Mqp, C, Mkp = _kv_shapes(who, q, k, vt)
    Mk = int(Mk)
    bias_rows = _key_rows(who, bias, "bias must be", q, B, Mk)
    out = _attention_out(q, k, vt, Mq, Mkp)
    _check(lib().vtm_attention_kv_bias(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1),
                                       out.data_ptr(), C, dtype_code(q), B, heads, Mq, Mqp, Mk, Mkp, C // heads, float(scale),
                                       *bias_rows, _stream()), "vtm_attention_kv_bias")
    return out


@_on_device
def frame_order(keep: torch.Tensor, inv_local: torch.Tensor, F: int, N: int
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The kept rows of a merge closure in frame order (vtm_frame_order, include/vidtome_hip.h): keep (B, M_l) int32, the
    distinct joined rows in [0, F N) of the merged tokens in any order, inv_local (B, F N) int32 with entries in [0, M_l) ->
    (keep_sorted (B, M_l) ascending, inv_sorted (B, F N) = the position in keep_sorted of keep[b, inv_local[b, i]], seg_off
    (B F + 1) int32: absolute offsets into the (B M_l)-row sequence of the rows whose kept token lies in frame f of sample
    b).  Integer, deterministic, nothing is read back."""
    _req(keep, "keep"), _req(inv_local, "inv_local")
    F, N = int(F), int(N)
    if keep.dim() != 2 or inv_local.dim() != 2 or keep.dtype != torch.int32 or inv_local.dtype != torch.int32 \
            or inv_local.device != keep.device or inv_local.shape[0] != keep.shape[0] or inv_local.shape[1] != F * N:
        raise RuntimeError("vidtome_amd: frame_order takes keep (B, M_l) and inv_local (B, F N), int32 on one device")
    B, Ml = keep.shape
    dev = keep.device
    keep_sorted = torch.empty_like(keep)
    inv_sorted = torch.empty_like(inv_local)
    seg_off = torch.empty((B * F + 1,), dtype=torch.int32, device=dev)
    nbytes = lib().vtm_frame_order_ws_bytes(B, F, N)
    ws = _workspace("frame_order", nbytes, dev)
    _check(lib().vtm_frame_order(_ptr(keep), Ml, _ptr(inv_local), B, F, N, _ptr(ws), nbytes, _ptr(keep_sorted),
                                 _ptr(inv_sorted), _ptr(seg_off), _stream()), "vtm_frame_order")
    return keep_sorted, inv_sorted, seg_off


@_on_device
def attention_kv_segments(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, seg_off: torch.Tensor,
                          max_seg_rows: int, Mk: int, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The cross-attention core over query segments (vtm_attention_kv_segments): q (rows, C) one row range, contiguous along
    the last axis; k (n_seg, Mkp, C) and vt (n_seg, C, ldvt >= Mk) as for attention_kv_bias, Mkp a multiple of 8; seg_off
    (n_seg + 1) int32 on q's device, absolute row offsets that never decrease; ``max_seg_rows`` a host bound on every
    segment's length.  Row i of segment s is softmax(q[i] K_s^T * scale) V_s; the result is (rows, C), rows outside every
    segment are not written (``out``: the buffer to write into).  fp16 / bf16 operands only."""
    _half_operands("attention_kv_segments", q, k, vt)
    if q.dim() != 2 or k.dim() != 3 or vt.dim() != 3 or not q.is_cuda or k.device != q.device or vt.device != q.device:
        raise RuntimeError("attention_kv_segments: q must be (rows, C), k (n_seg, Mkp, C) and vt (n_seg, C, ldvt) on one GPU")
    rows, C = q.shape
    n_seg, Mkp = k.shape[0], k.shape[1]
    heads, Mk = int(heads), int(Mk)
    if heads < 1 or C % heads or k.shape[2] != C or vt.shape[0] != n_seg or vt.shape[1] != C or q.stride(1) != 1 \
            or k.stride(2) != 1 or vt.stride(2) != 1 or k.stride(0) != Mkp * k.stride(1) or vt.stride(0) != C * vt.stride(1):
        raise RuntimeError("attention_kv_segments: k must be (n_seg, Mkp, C) and vt (n_seg, C, ldvt), dense over the segments")
    if not isinstance(seg_off, torch.Tensor) or seg_off.dtype != torch.int32 or seg_off.device != q.device \
            or seg_off.dim() != 1 or seg_off.numel() != n_seg + 1 or not seg_off.is_contiguous():
        raise RuntimeError("attention_kv_segments: seg_off must be (n_seg + 1,) int32 on q's device")
    if out is None:
        out = torch.empty((rows, C), dtype=q.dtype, device=q.device)
    elif out.shape != (rows, C) or out.dtype != q.dtype or out.device != q.device or out.stride(1) != 1:
        raise RuntimeError("attention_kv_segments: out must be (rows, C) like q")
    _check(lib().vtm_attention_kv_segments(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(1), vt.data_ptr(), vt.stride(1),
                                           out.data_ptr(), out.stride(0), dtype_code(q), rows, seg_off.data_ptr(), n_seg,
                                           int(max_seg_rows), heads, Mk, Mkp, C // heads, float(scale), _stream()),
           "vtm_attention_kv_segments")
    return out


@_on_device
def attention_probs(q: torch.Tensor, k: torch.Tensor, heads: int, Mq: int, Mk: int, scale: float,
                    bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The head-averaged probabilities of the cross-attention core (vtm_attention_probs): q (B, Mqp, C) and k (B, Mkp, C)
    views contiguous along the last axis as for attention_kv_bias, fp16 / bf16; ``bias`` None or what attention_kv_bias
    takes.  Returns mean_head softmax(q K^T * scale + bias) of the first Mq query rows and Mk <= 256 keys, a new
    (B, Mq, Mk) float32 tensor.  No V operand, no (B, heads, Mq, Mk) intermediate; deterministic."""
    who = "attention_probs"
    B, Mqp, C, Mkp, heads, Mq, Mk = _qk_views(who, q, k, heads, Mq, Mk, dense_single=True)
    bias_rows = _key_rows(who, bias, "bias must be None or", q, B, Mk, optional=True)
    out = torch.empty((B, Mq, Mk), dtype=torch.float32, device=q.device)
    _check(lib().vtm_attention_probs(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), out.data_ptr(), Mk, dtype_code(q),
                                     B, heads, Mq, Mqp, Mk, Mkp, C // heads, float(scale), *bias_rows, _stream()),
           "vtm_attention_probs")
    return out


@_on_device
def attention_word_map(q: torch.Tensor, k: torch.Tensor, heads: int, Mq: int, Mk: int, scale: float, weights: torch.Tensor,
                       out: torch.Tensor, out_rows: Optional[torch.Tensor] = None, accumulate: bool = True,
                       bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One weighted column sum of the head-averaged cross-attention map, added in place (vtm_attention_word_map): q, k,
    heads, Mq, Mk, scale and ``bias`` as for attention_probs (any head count); ``weights`` fp32 on q's device, (B, >= Mk) with
    a row per sample or (1, >= Mk) with one row for all, finite (the caller's business).  ``out`` is fp32 (R, >= Mq) on q's
    device with unit stride along the row: sample b goes to row ``out_rows[b]`` (int64 (B,) on q's device, distinct rows
    inside ``out``: the caller's business) or to row b.  ``accumulate``: add to what ``out`` holds, else overwrite.  Returns
    ``out``.  One launch; no (B, Mq, Mk) map, deterministic."""
    who = "attention_word_map"
    B, Mqp, C, Mkp, heads, Mq, Mk = _qk_views(who, q, k, heads, Mq, Mk, dense_single=False)
    if weights is None:
        raise RuntimeError(f"{who}: weights are required")
    b_ptr, ld_bias, b_stride = _key_rows(who, bias, "bias must be", q, B, Mk, optional=True)
    w_ptr, ld_w, w_stride = _key_rows(who, weights, "weights must be", q, B, Mk)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != q.device or out.dim() != 2 \
            or out.shape[1] < Mq or out.stride(1) != 1 or (out.shape[0] > 1 and out.stride(0) < out.shape[1]):
        raise RuntimeError(f"{who}: out must be fp32 (rows, >= Mq) on q's device, contiguous along its last axis")
    if out_rows is None:
        if out.shape[0] < B:
            raise RuntimeError(f"{who}: out has {out.shape[0]} rows for {B} samples")
    elif not isinstance(out_rows, torch.Tensor) or out_rows.dtype != torch.int64 or out_rows.device != q.device \
            or tuple(out_rows.shape) != (B,) or not out_rows.is_contiguous():
        raise RuntimeError(f"{who}: out_rows must be a contiguous int64 (B,) tensor on q's device")
    _check(lib().vtm_attention_word_map(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), dtype_code(q), B, heads, Mq, Mqp,
                                        Mk, Mkp, C // heads, float(scale), b_ptr, ld_bias, b_stride, w_ptr, ld_w, w_stride,
                                        out.data_ptr(), out.stride(0) if out.shape[0] > 1 else out.shape[1], _ptr(out_rows),
                                        1 if accumulate else 0, _stream()), "vtm_attention_word_map")
    return out


LOCAL_BLEND_MAX_GROUPS, LOCAL_BLEND_MAX_POOL = 8, 3   # what vtm_local_blend takes (csrc/local_blend.hip)


@_on_device
def local_blend(acc: torch.Tensor, x: torch.Tensor, x_src: torch.Tensor, pool: int, threshold: float,
                out: Optional[torch.Tensor] = None, return_mask: bool = False):
    """The LocalBlend tail (vtm_local_blend): ``acc`` (G, F, h, w) fp32 accumulated word maps, ``x`` / ``x_src`` (F, C, H, W)
    contiguous latents of one dtype, H % h == 0 and W % w == 0.  A pixel is inside the mask when, for any group, the maximum
    of the map over the (2 pool + 1)^2 window around its cell exceeds ``threshold`` times the map's maximum; ``out`` takes x
    inside and x_src outside.  ``out`` None: a new tensor; it may be x.  Returns out, or (out, mask uint8 (F, H, W))."""
    who = "local_blend"
    if not isinstance(acc, torch.Tensor) or acc.dtype != torch.float32 or acc.dim() != 4 or not acc.is_cuda \
            or not acc.is_contiguous() or not 1 <= acc.shape[0] <= LOCAL_BLEND_MAX_GROUPS:
        raise RuntimeError(f"{who}: acc must be a contiguous fp32 (G <= {LOCAL_BLEND_MAX_GROUPS}, F, h, w) tensor on the GPU")
    G, F, h, w = acc.shape
    for t, name in ((x, "x"), (x_src, "x_src")):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.device != acc.device or not t.is_contiguous() \
                or t.dtype not in _DT or t.dtype != x.dtype or t.shape != x.shape:
            raise RuntimeError(f"{who}: {name} must be a contiguous (F, C, H, W) fp16 / bf16 / fp32 tensor on acc's device, "
                               "x and x_src alike")
    if x.shape[0] != F or x.shape[2] % h or x.shape[3] % w:
        raise RuntimeError(f"{who}: latents {tuple(x.shape)} do not fit maps {tuple(acc.shape)} (F frames, H % h == W % w == 0)")
    pool = int(pool)
    if not 0 <= pool <= LOCAL_BLEND_MAX_POOL:
        raise RuntimeError(f"{who}: pool = {pool}, a radius of 0 .. {LOCAL_BLEND_MAX_POOL} is taken")
    if out is None:
        out = torch.empty_like(x)
    elif not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device \
            or not out.is_contiguous():
        raise RuntimeError(f"{who}: out must be a contiguous tensor like x")
    _, C, H, W = x.shape
    mask = torch.empty((F, H, W), dtype=torch.uint8, device=x.device) if return_mask else None
    _check(lib().vtm_local_blend(acc.data_ptr(), G, F, h, w, x.data_ptr(), x_src.data_ptr(), out.data_ptr(), dtype_code(x), C,
                                 H, W, pool, float(threshold), _ptr(mask), _stream()), "vtm_local_blend")
    return (out, mask) if return_mask else out


KEY_MASS_MAX_KEYS, KEY_MASS_MAX_QUERIES = 4096, 65536   # what vtm_attention_key_mass takes (csrc/attention_mass.hip)


@_on_device
def attention_key_mass(q: torch.Tensor, k: torch.Tensor, heads: int, Mq: int, Mk: int, scale: float,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-key attention mass of a self-attention call (vtm_attention_key_mass): q (B, Mqp, C) and k (B, Mkp, C) views
    contiguous along the last axis as for attention_probs, fp16 / bf16 -- the q | k column ranges of one (B, N, 3 C) buffer
    will do.  Returns sum_{i < Mq} mean_head softmax(q K^T * scale)[i, :], fp32 (B, Mk): a new tensor, or the first Mk columns
    of ``out`` (fp32 (B, >= Mk) on q's device, unit stride along the row; columns >= Mk are not written).  Mk <= 4096,
    Mq <= 65536, any head count; query rows >= Mq contribute exactly 0.  No V operand, no (B, Mq, Mk) intermediate;
    deterministic, a sample's bits do not depend on B.  More than 128 queries go through a cached workspace."""
    who = "attention_key_mass"
    B, Mqp, C, Mkp, heads, Mq, Mk = _qk_views(who, q, k, heads, Mq, Mk, dense_single=False)
    if Mk > KEY_MASS_MAX_KEYS or Mq > KEY_MASS_MAX_QUERIES:
        raise RuntimeError(f"{who}: Mk = {Mk}, Mq = {Mq}: at most {KEY_MASS_MAX_KEYS} keys and {KEY_MASS_MAX_QUERIES} queries "
                           "are taken")
    if out is None:
        out = torch.empty((B, Mk), dtype=torch.float32, device=q.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != q.device or out.dim() != 2 \
            or out.shape[0] != B or out.shape[1] < Mk or out.stride(1) != 1 or (B > 1 and out.stride(0) < out.shape[1]):
        raise RuntimeError(f"{who}: out must be fp32 (B, >= Mk) on q's device, contiguous along its last axis")
    nbytes = lib().vtm_attention_key_mass_ws_bytes(B, Mq, Mk)
    ws = _workspace("key_mass", nbytes, q.device) if nbytes else None
    _check(lib().vtm_attention_key_mass(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), out.data_ptr(),
                                        out.stride(0) if B > 1 else out.shape[1], dtype_code(q), B, heads, Mq, Mqp, Mk, Mkp,
                                        C // heads, float(scale), _ptr(ws), nbytes, _stream()), "vtm_attention_key_mass")
    return out


SAG_MAX_RADIUS, SAG_MAX_PLANE = 4, 16384   # what vtm_sag_degrade takes (csrc/sag.hip)


def gaussian_taps(radius: int, sigma: float):
    """The 2 radius + 1 taps exp(-0.5 (k / sigma)^2) of vtm_sag_degrade's blur: computed in float64, normalised to sum 1, then
    rounded to fp32 (returned as Python floats that are fp32 values)."""
    radius, sigma = int(radius), float(sigma)
    if radius < 0 or not sigma > 0.0:
        raise RuntimeError(f"gaussian_taps: radius = {radius}, sigma = {sigma}: a radius >= 0 and a sigma > 0 are taken")
    w = [math.exp(-0.5 * (k / sigma) ** 2) for k in range(-radius, radius + 1)]
    total = math.fsum(w)
    return [_f32_round(v / total) for v in w]


def _chunk_out(who: str, out, shape, ref: torch.Tensor, ref_name: str, like: str, ids):
    """The chunk-local result of sag_degrade / semantic_guidance: ``out`` when given -- a contiguous tensor of ``shape`` with
    ``ref``'s dtype and device that does not overlap ref -- else a new one; and the frame ids _frame_rows left, on ref's
    device (a list is uploaded).  Returns (out, ids)."""
    if isinstance(ids, torch.Tensor) and _req(ids, "frame_ids").device != ref.device:
        raise RuntimeError(f"{who}: frame_ids lives on {ids.device}, {ref_name} on {ref.device}")
    if out is None:
        out = torch.empty(shape, dtype=ref.dtype, device=ref.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != ref.dtype or out.device != ref.device \
            or not out.is_contiguous():
        raise RuntimeError(f"{who}: out must be a contiguous ({', '.join(map(str, shape))}) tensor of {like}")
    else:
        r_lo, o_lo = ref.data_ptr(), out.data_ptr()
        if o_lo < r_lo + ref.numel() * ref.element_size() and r_lo < o_lo + out.numel() * out.element_size():
            raise RuntimeError(f"{who}: out overlaps {ref_name}")
    if isinstance(ids, list):
        ids = torch.tensor(ids, dtype=torch.int32, device=ref.device)
    return out, ids


@_on_device
def sag_degrade(x: torch.Tensor, model_out: torch.Tensor, mass: torch.Tensor, h_m: int, w_m: int, sqrt_alpha: float,
                sqrt_beta: float, taps, threshold: float = 1.0, *, groups: int = 1, group: int = 0, frame_ids=None,
                pred_type: int = PRED_EPSILON, out: Optional[torch.Tensor] = None, want_mask: bool = False):
    """The degrade step of self-attention guidance for one chunk (vtm_sag_degrade, include/vidtome_hip.h): ``x``
    (n_frames, C, H, W) the whole-video latents, ``model_out`` (groups * F, C, H, W) the UNet output of the chunk, group-major
    -- group ``group`` of it is read; ``frame_ids`` as for guided_step; ``mass`` fp32 (F, >= h_m * w_m) on x's device, unit
    stride along the row (attention_key_mass of the mid block's (h_m, w_m) grid); ``taps`` the 2 r + 1 blur taps, r <= 4
    (gaussian_taps).  Returns out, a chunk-local (F, C, H, W) tensor of x's dtype (``out``: a contiguous tensor of that shape
    that does not overlap x, or None for a new one), or (out, mask uint8 (F, H, W)) with ``want_mask``."""
    who = "sag_degrade"
    groups, group, pred_type, h_m, w_m = int(groups), int(group), int(pred_type), int(h_m), int(w_m)
    for t, name in ((x, "x"), (model_out, "model_out")):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.dtype not in _DT:
            raise RuntimeError(f"{who}: {name} must be a (frames, C, H, W) fp16 / bf16 / fp32 tensor")
    if pred_type not in (PRED_EPSILON, PRED_V, PRED_SAMPLE):
        raise RuntimeError(f"{who}: unknown pred_type {pred_type}")
    if groups < 1 or not 0 <= group < groups:
        raise RuntimeError(f"{who}: groups = {groups}, group = {group}: a group index outside [0, groups)")
    taps = [float(t) for t in taps]
    if len(taps) % 2 != 1 or len(taps) > 2 * SAG_MAX_RADIUS + 1:
        raise RuntimeError(f"{who}: {len(taps)} taps: 2 r + 1 of them are taken, r <= {SAG_MAX_RADIUS}")
    r = len(taps) // 2
    first, ids, F = _frame_rows(frame_ids, x.shape[0], who)
    _, C, H, W = x.shape
    if model_out.shape[0] != groups * F or tuple(model_out.shape[1:]) != (C, H, W):
        raise RuntimeError(f"{who}: model_out {tuple(model_out.shape)} is not ({groups} groups * {F} frames, {C}, {H}, {W})")
    if model_out.dtype != x.dtype or model_out.device != x.device:
        raise RuntimeError(f"{who}: model_out ({model_out.dtype}, {model_out.device}) is not like x ({x.dtype}, {x.device})")
    if H * W > SAG_MAX_PLANE:
        raise RuntimeError(f"{who}: frames of {H} x {W} latents: a plane of at most {SAG_MAX_PLANE} elements (128 x 128) is "
                           "taken, two fp32 planes of it live in a workgroup's LDS")
    if H <= r or W <= r:
        raise RuntimeError(f"{who}: reflect padding of radius {r} needs H, W > {r}")
    if not isinstance(mass, torch.Tensor) or mass.dtype != torch.float32 or mass.device != x.device or mass.dim() != 2 \
            or mass.shape[0] != F or mass.shape[1] < h_m * w_m or mass.stride(1) != 1 \
            or (F > 1 and mass.stride(0) < mass.shape[1]) or h_m < 1 or w_m < 1 or h_m > H or w_m > W:
        raise RuntimeError(f"{who}: mass must be fp32 ({F}, >= h_m * w_m = {h_m * w_m}) on x's device, contiguous along its "
                           f"last axis, with the ({h_m}, {w_m}) grid inside ({H}, {W})")
    _req(x, "x"), _req(model_out, "model_out")
    out, ids = _chunk_out(who, out, (F, C, H, W), x, "x", "x's dtype on x's device", ids)
    mask = torch.empty((F, H, W), dtype=torch.uint8, device=x.device) if want_mask else None
    if F == 0:
        return (out, mask) if want_mask else out
    E = C * H * W
    _check(lib().vtm_sag_degrade(x.data_ptr() + first * E * x.element_size(), x.shape[0] - first, _ptr(ids),
                                 model_out.data_ptr() + group * F * E * x.element_size(), mass.data_ptr(),
                                 mass.stride(0) if F > 1 else mass.shape[1], h_m, w_m, dtype_code(x), F, C, H, W, pred_type,
                                 float(sqrt_alpha), float(sqrt_beta), (_f32 * len(taps))(*taps), r, float(threshold),
                                 out.data_ptr(), _ptr(mask), _stream()), "vtm_sag_degrade")
    return (out, mask) if want_mask else out


SEGA_MAX_CONCEPTS, SEGA_MAX_PLANE = 6, 16384    # include/vidtome_hip.h VTM_SEGA_MAX_CONCEPTS, VTM_SEGA_MAX_PLANE
SEGA_CHANNEL, SEGA_SUM, SEGA_REGION, SEGA_CHANNEL_REGION, SEGA_SUM_REGION = range(5)   # VTM_SEGA_*: a concept's mask mode


def sega_rank(q: float, P: int) -> Tuple[int, float]:
    """(rank_lo, rank_frac) of vtm_semantic_guidance for the quantile ``q`` in [0, 1] of a population of ``P`` values:
    pos = q (P - 1) in double, rank_lo = floor(pos), rank_frac = pos - rank_lo."""
    q, P = float(q), int(P)
    if not 0.0 <= q <= 1.0 or P < 1:
        raise RuntimeError(f"sega_rank: q = {q}, P = {P}: a quantile inside [0, 1] of at least one value is taken")
    pos = q * (P - 1)
    lo = min(int(math.floor(pos)), P - 1)
    return lo, pos - lo


@_on_device
def semantic_guidance(model_out: torch.Tensor, groups: int, g_uncond: int, g_cond: int, guidance_scale: float, group, scale,
                      threshold, w_apply, w_acc, mode, *, regions: Optional[torch.Tensor] = None,
                      momentum: Optional[torch.Tensor] = None, frame_ids=None, mom_scale: float = 0.0, mom_beta: float = 0.0,
                      mom_apply: bool = False, out: Optional[torch.Tensor] = None, want_masks: bool = False):
    """Semantic guidance for one chunk (vtm_semantic_guidance, include/vidtome_hip.h): ``model_out`` (groups * F, C, H, W),
    group-major; ``g_uncond`` / ``g_cond`` (-1: no classifier-free term) the groups of u and c; per concept one host number
    in each of ``group``, ``scale`` (signed), ``threshold`` (the quantile q in [0, 1]; the ranks are sega_rank's), ``w_apply``,
    ``w_acc`` and ``mode`` (SEGA_*); ``regions`` uint8 (E, F, H, W), needed where a live concept's mode names a region;
    ``momentum`` the whole-video fp32 (n_frames, C, H, W) buffer, updated in place at the rows ``frame_ids`` names (as for
    guided_step; without momentum F is model_out's frame count and frame_ids only gives it).  Returns out, a chunk-local
    (F, C, H, W) tensor of model_out's dtype (``out``: a contiguous tensor of that shape that does not overlap model_out, or
    None for a new one), or (out, masks uint8 (E, F, C, H, W)) with ``want_masks`` -- rows of concepts whose two weights are
    0 are not written."""
    who = "semantic_guidance"
    groups, g_uncond, g_cond = int(groups), int(g_uncond), int(g_cond)
    if not isinstance(model_out, torch.Tensor) or model_out.dim() != 4 or model_out.dtype not in _DT:
        raise RuntimeError(f"{who}: model_out must be a (groups * frames, C, H, W) fp16 / bf16 / fp32 tensor")
    cols = [list(v) for v in (group, scale, threshold, w_apply, w_acc, mode)]
    E = len(cols[0])
    if any(len(c) != E for c in cols) or E > SEGA_MAX_CONCEPTS:
        raise RuntimeError(f"{who}: {[len(c) for c in cols]} per-concept values: one of each for 0 .. {SEGA_MAX_CONCEPTS} concepts")
    group, mode = [int(v) for v in cols[0]], [int(v) for v in cols[5]]
    scale, threshold, w_apply, w_acc = ([float(v) for v in c] for c in cols[1:5])
    if not 1 <= groups <= SOLVER_MAX_GROUPS or not 0 <= g_uncond < groups or not -1 <= g_cond < groups \
            or any(not 0 <= g < groups for g in group):
        raise RuntimeError(f"{who}: groups = {groups} (1 .. {SOLVER_MAX_GROUPS}), g_uncond = {g_uncond}, g_cond = {g_cond}, "
                           f"group = {group}: a group index outside [0, groups)")
    if any(m not in range(5) for m in mode):
        raise RuntimeError(f"{who}: mode = {mode}: SEGA_CHANNEL .. SEGA_SUM_REGION (0 .. 4) are taken")
    if any(not 0.0 <= q <= 1.0 for q in threshold):
        raise RuntimeError(f"{who}: threshold = {threshold}: quantiles inside [0, 1] are taken")
    guidance_scale, mom_scale, mom_beta = float(guidance_scale), float(mom_scale), float(mom_beta)
    if not all(math.isfinite(v) for v in w_apply + w_acc + [guidance_scale, mom_scale, mom_beta]):
        raise RuntimeError(f"{who}: the weights, guidance_scale, mom_scale and mom_beta must be finite")
    if model_out.shape[0] % groups:
        raise RuntimeError(f"{who}: model_out has {model_out.shape[0]} samples, not {groups} groups of frames")
    n_chunk, C, H, W = model_out.shape[0] // groups, *model_out.shape[1:]
    if momentum is not None:
        if not isinstance(momentum, torch.Tensor) or momentum.dim() != 4 or momentum.dtype != torch.float32 \
                or tuple(momentum.shape[1:]) != (C, H, W) or momentum.device != model_out.device:
            raise RuntimeError(f"{who}: momentum must be an fp32 (frames, {C}, {H}, {W}) tensor on model_out's device")
        first, ids, F = _frame_rows(frame_ids, momentum.shape[0], who)
    else:
        first, ids, F = 0, None, n_chunk if frame_ids is None else len(frame_ids)
    if F != n_chunk:
        raise RuntimeError(f"{who}: model_out {tuple(model_out.shape)} is not ({groups} groups * {F} frames, C, H, W)")
    if C < 1 or H < 1 or W < 1 or H * W > SEGA_MAX_PLANE:
        raise RuntimeError(f"{who}: frames of {C} x {H} x {W} latents: a plane of 1 .. {SEGA_MAX_PLANE} elements (128 x 128) is "
                           "taken, it lives in a workgroup's LDS")
    live = [e for e in range(E) if _f32_round(w_apply[e]) != 0.0 or _f32_round(w_acc[e]) != 0.0]
    if any(mode[e] >= SEGA_REGION for e in live):
        if not isinstance(regions, torch.Tensor) or regions.dtype != torch.uint8 or tuple(regions.shape) != (E, F, H, W) \
                or regions.device != model_out.device:
            raise RuntimeError(f"{who}: a region mode needs regions, a uint8 ({E}, {F}, {H}, {W}) tensor on model_out's device")
    elif regions is not None and not isinstance(regions, torch.Tensor):
        raise RuntimeError(f"{who}: regions must be a tensor")
    _req(model_out, "model_out")
    for t, name in ((regions, "regions"), (momentum, "momentum")):
        if t is not None and _req(t, name).device != model_out.device:
            raise RuntimeError(f"{who}: {name} lives on {t.device}, model_out on {model_out.device}")
    out, ids = _chunk_out(who, out, (F, C, H, W), model_out, "model_out", "model_out's dtype on its device", ids)
    masks = torch.empty((E, F, C, H, W), dtype=torch.uint8, device=model_out.device) if want_masks else None
    if F == 0:
        return (out, masks) if want_masks else out
    ranks = [sega_rank(q, H * W) for q in threshold]
    i32, n = ctypes.c_int32 * max(E, 1), max(E, 1)
    _check(lib().vtm_semantic_guidance(
        model_out.data_ptr(), dtype_code(model_out), F, C, H, W, groups, g_uncond, g_cond, guidance_scale, E, i32(*group),
        (_f32 * n)(*scale), i32(*(r[0] for r in ranks)), (ctypes.c_double * n)(*(r[1] for r in ranks)), (_f32 * n)(*w_apply),
        (_f32 * n)(*w_acc), i32(*mode), _ptr(regions),
        momentum.data_ptr() + first * C * H * W * 4 if momentum is not None else None,
        momentum.shape[0] - first if momentum is not None else 0, _ptr(ids), mom_scale, mom_beta, int(bool(mom_apply)),
        out.data_ptr(), _ptr(masks), _stream()), "vtm_semantic_guidance")
    return (out, masks) if want_masks else out


FREEU_MAX_PLANE = 16384                         # what vtm_freeu takes (csrc/freeu.hip): H * W of a plane


def freeu_lanes(P: int) -> int:
    """The lanes that own one plane of ``P`` elements in vtm_freeu's apply launch (16 / 64 / 256 / 1024): the kernel form, the
    library's own rule (vtm_freeu_lanes), a function of P alone.  0 for a P outside [4, FREEU_MAX_PLANE]."""
    return int(lib().vtm_freeu_lanes(int(P)))


def freeu_rounding_counts(P: int, C_h: int) -> Tuple[int, int]:
    """(K_s, K_m) of csrc/freeu.hip's header, in units of 2^-24: the roundings between an input value and a stored skip-plane
    value, folded for the error form ``K_s 2^-24 (|v| + |s - 1| 4 sum|v| / P)``, and the roundings between an input value
    and an entry of version 2's channel-mean map."""
    P, C_h = int(P), int(C_h)
    G = freeu_lanes(P)
    if G == 0 or C_h < 2:
        raise ValueError(f"freeu_rounding_counts: P = {P}, C_h = {C_h}: 4 <= P <= {FREEU_MAX_PLANE} and C_h >= 2 are taken")
    chunks = -(-P // 8)
    R = 8 * -(-chunks // G) + int(math.log2(min(G, 64))) + (G // 64 if G > 64 else 0)
    return -(-(7 * R + 180) // 4) + 1, -(-C_h // 16) + 15


@_on_device
def freeu(x: torch.Tensor, C_h: int, b: float, s: float, version: int = 1) -> torch.Tensor:
    """FreeU in place on ``x`` (vtm_freeu, include/vidtome_hip.h): the contiguous (B, C_h + C_s, H, W) concatenation
    cat([hidden_states, res_hidden_states], 1) of an up-block resnet, fp16 / bf16 / fp32 on the GPU.  Planes c < C_h // 2 are
    scaled by ``b`` (``version`` 1, Diffusers) or by the original repository's per-pixel gain (``version`` 2), planes
    C_h // 2 <= c < C_h are not touched, planes c >= C_h get their four lowest frequency bins scaled by ``s``.  Launches on
    the current stream; version 2 takes its workspace from the per-stream cache.  Returns ``x``."""
    who = "freeu"
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{who}: x must be a (B, C_h + C_s, H, W) tensor")
    if x.dtype not in _DT:
        raise ValueError(f"{who}: x is {x.dtype}: fp16, bf16 and fp32 are taken")
    if not x.is_contiguous():
        raise ValueError(f"{who}: x must be contiguous NCHW (strides {tuple(x.stride())} of shape {tuple(x.shape)} are not)")
    C_h, version, b, s = int(C_h), int(version), float(b), float(s)
    B, C, H, W = x.shape
    if version not in (1, 2):
        raise ValueError(f"{who}: version = {version}: 1 (Diffusers) or 2 (the original repository) is taken")
    if C_h < 2 or C - C_h < 1:
        raise ValueError(f"{who}: C_h = {C_h} of {C} channels: C_h >= 2 and C_s = C - C_h >= 1 are taken")
    if H < 2 or W < 2 or H * W > FREEU_MAX_PLANE:
        raise ValueError(f"{who}: x has planes of {H} x {W}: H, W >= 2 and H * W <= FREEU_MAX_PLANE = {FREEU_MAX_PLANE} are "
                         "taken")
    if not x.is_cuda:
        raise ValueError(f"{who}: x lives on {x.device}: it must live on the GPU (vidtome_amd has no CPU path)")
    if B == 0:
        return x
    nbytes = lib().vtm_freeu_ws_bytes(B, H * W, version)
    ws = _workspace("freeu", nbytes, x.device) if nbytes else None
    _check(lib().vtm_freeu(x.data_ptr(), dtype_code(x), B, C_h, C - C_h, H, W, b, s, version, _ptr(ws), nbytes, _stream()),
           "vtm_freeu")
    return x


@_on_device
def compact_queries(loc: torch.Tensor, U: int, Nd: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """loc (B, Ml) merged position of every local token -> (qc (B, Ml) distinct positions, tmap (B, Ml) row of qc each
    local token reads, count (B,) number of distinct positions); see include/vidtome_hip.h."""
    _req(loc, "loc")
    B, Ml = loc.shape
    i32 = dict(dtype=torch.int32, device=loc.device)
    qc, tmap, count = torch.empty((B, Ml), **i32), torch.empty((B, Ml), **i32), torch.empty((B,), **i32)
    nb = int(lib().vtm_compact_queries_ws_bytes(B, Nd))
    ws = _workspace("compact", nb, loc.device)
    _check(lib().vtm_compact_queries(_ptr(loc), B, Ml, U, Nd, _ptr(ws), nb, _ptr(qc), _ptr(tmap), _ptr(count), _stream()),
           "vtm_compact_queries")
    return qc, tmap, count


@_on_device
def fold_keys(cur: torch.Tensor, L: int, cid: torch.Tensor, n_ids: int, dtype: torch.dtype
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """cur (B, M) pool row of every merged position (rows >= L: anchor row cur - L), cid (B, Ma) content id of every anchor
    row (< n_ids; equal ids = identical rows) -> (key_sel (B, M) surviving positions, k_bias (B, Mp) int32 words holding
    log2(copies) as a 16-bit (hi, lo) pair of ``dtype``, k_count (B,)); see include/vidtome_hip.h."""
    _req(cur, "cur")
    _req(cid, "cid")
    B, M = cur.shape
    Mp = (M + 7) // 8 * 8
    i32 = dict(dtype=torch.int32, device=cur.device)
    key_sel, k_bias, k_count = torch.empty((B, M), **i32), torch.empty((B, Mp), **i32), torch.empty((B,), **i32)
    code = {torch.float16: 1, torch.bfloat16: 2}[dtype]
    nb = int(lib().vtm_fold_keys_ws_bytes(B, M, n_ids))
    ws = _workspace("fold", nb, cur.device)
    _check(lib().vtm_fold_keys(_ptr(cur), B, M, L, _ptr(cid), cid.shape[1], n_ids, code, _ptr(ws), nb, _ptr(key_sel),
                               _ptr(k_bias), Mp, _ptr(k_count), _stream()), "vtm_fold_keys")
    return key_sel, k_bias, k_count


@_on_device
def geglu(x: torch.Tensor) -> torch.Tensor:
    """value * gelu(gate) over the two halves of the last axis (the GEGLU feed-forward, patch.py:187-199)."""
    _req(x, "x")
    D = x.shape[-1] // 2
    xc = x.contiguous()
    out = torch.empty(xc.shape[:-1] + (D,), dtype=x.dtype, device=x.device)
    _check(lib().vtm_geglu(_ptr(xc), dtype_code(xc), xc.numel() // (2 * D), D, _ptr(out), _stream()), "vtm_geglu")
    return out


@_on_device
def groupnorm_silu(x: torch.Tensor, groups: int, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float,
                   add: Optional[torch.Tensor] = None, act: bool = True) -> torch.Tensor:
    """act(GroupNorm(x [+ add[:, :, None, None]])) on a contiguous NCHW tensor in one launch (pnp_utils.py:113-114 and
    :133-142); ``add`` is the (B, C) projected time embedding, ``act`` selects SiLU."""
    _req(x, "x")
    B, C = x.shape[0], x.shape[1]
    for name, p, shape in (("weight", weight, (C,)), ("bias", bias, (C,)), ("add", add, (B, C))):
        if p is not None and (p.dtype != x.dtype or tuple(p.shape) != shape or p.device != x.device or not p.is_contiguous()):
            raise RuntimeError(f"vidtome_amd: groupnorm_silu {name} must be a contiguous {shape} {x.dtype} tensor on {x.device}")
    out = torch.empty_like(x)
    _check(lib().vtm_groupnorm_silu(_ptr(x), _ptr(add), _ptr(weight), _ptr(bias), dtype_code(x), B, C,
                                    x.numel() // max(B * C, 1), int(groups), float(eps), int(bool(act)), _ptr(out), _stream()),
           "vtm_groupnorm_silu")
    return out


@_on_device
def resnet_tail(shortcut: torch.Tensor, hidden: torch.Tensor, inject_rows: int, period: int, scale: float) -> torch.Tensor:
    """(shortcut + hidden[row(b)]) / scale, bit-identical to the torch expression (pnp_utils.py:146-162): output row b adds
    compact row ``b % period`` of ``hidden`` for b < inject_rows, else row ``b - inject_rows + period``."""
    _req(shortcut, "shortcut"), _req(hidden, "hidden")
    B = shortcut.shape[0]
    M = shortcut.numel() // max(B, 1)
    rows = B if inject_rows == 0 else period + B - inject_rows
    if hidden.dtype != shortcut.dtype or hidden.device != shortcut.device or tuple(hidden.shape) != (rows,) + tuple(shortcut.shape[1:]):
        raise RuntimeError(f"vidtome_amd: resnet_tail hidden must be {(rows,) + tuple(shortcut.shape[1:])} {shortcut.dtype}, "
                           f"got {tuple(hidden.shape)} {hidden.dtype}")
    out = torch.empty_like(shortcut)
    _check(lib().vtm_resnet_tail(_ptr(shortcut), _ptr(hidden), dtype_code(shortcut), B, M, int(inject_rows), int(period),
                                 float(scale), _ptr(out), _stream()), "vtm_resnet_tail")
    return out


@_on_device
def linear_rows(x0: torch.Tensor, x1: Optional[torch.Tensor], rows: Optional[torch.Tensor],
                rows2: Optional[torch.Tensor], n: int, weight: torch.Tensor, bias: Optional[torch.Tensor],
                transposed: bool = False, pad_to: int = 8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b, i] = pool[b, rows[b, rows2[b, i]]] @ weight^T (+ bias) for i < n (either map may be None = identity).
    Returns (B, n_pad, N) token-major, or (B, N, n_pad) channel-major when ``transposed`` (n_pad = n rounded up to
    ``pad_to``; the padding rows / columns are zero when this function allocates the result -- consumers such as a
    gate multiply or a later GEMM then see finite values -- and left alone in a preallocated ``out`` view, last axis
    contiguous)."""
    _req(x0, "x0"), _req(weight, "weight")
    B, P0, K = x0.shape
    P1 = 0 if x1 is None else _req(x1, "x1").shape[1]
    N = weight.shape[0]
    if weight.shape[1] != K or weight.dtype != x0.dtype:
        raise RuntimeError("linear_rows: weight must be (N, K) in the token dtype")
    if rows is not None:
        _req(rows, "rows")
    if rows2 is not None:
        _req(rows2, "rows2")
    n_pad = (n + pad_to - 1) // pad_to * pad_to
    if out is None:
        out = torch.empty((B, N, n_pad) if transposed else (B, n_pad, N), dtype=x0.dtype, device=x0.device)
        if n_pad != n:
            (out[:, :, n:] if transposed else out[:, n:]).zero_()
    if out.stride(2) != 1:
        raise RuntimeError("linear_rows: out must be contiguous along its last axis")
    _check(lib().vtm_linear_rows(_ptr(x0), P0, _ptr(x1), P1, dtype_code(x0), B, K, _ptr(rows),
                                 0 if rows is None else rows.shape[1], _ptr(rows2), n, _ptr(weight),
                                 _ptr(bias.contiguous() if bias is not None else None), N, out.data_ptr(), out.stride(1),
                                 out.stride(0), int(transposed), _stream()), "vtm_linear_rows")
    return out


LINEAR_NONE, LINEAR_RESID, LINEAR_GEGLU = 0, 1, 2          # vtm_linear_f32 epilogues
_EPILOGUES = {"none": LINEAR_NONE, "resid": LINEAR_RESID, "geglu": LINEAR_GEGLU}


@_on_device
def linear_f32(x0: torch.Tensor, x1: Optional[torch.Tensor], rows: Optional[torch.Tensor],
               rows2: Optional[torch.Tensor], n: int, weight: torch.Tensor, bias: Optional[torch.Tensor],
               epilogue: str = "none", resid: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32,
               transposed: bool = False, pad_to: int = 8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fp32 projections (csrc/linear_f32.hip): out[b, i] = pool[b, rows[b, rows2[b, i]]] @ weight^T (+ bias) for i < n,
    then ``epilogue`` "none", "resid" (+ ``resid``, laid out like the result) or "geglu" (weight = [value; gate] rows:
    value * gelu(gate), D = N / 2 channels).  fp32 tokens, weight and bias; the result is fp32 or, with ``out_dtype`` fp16,
    rounded once at the store.  Shapes and padding as linear_rows: (B, n_pad, N_out) token-major, or (B, N_out, n_pad)
    channel-major when ``transposed`` (the padding is zero when this function allocates the result)."""
    _req(x0, "x0"), _req(weight, "weight")
    B, P0, K = x0.shape
    P1 = 0 if x1 is None else _req(x1, "x1").shape[1]
    N = weight.shape[0]
    if x0.dtype != torch.float32 or weight.dtype != torch.float32 or weight.shape[1] != K \
            or (x1 is not None and x1.dtype != torch.float32):
        raise RuntimeError("linear_f32: tokens and weight must be fp32, weight (N, K)")
    if out_dtype not in (torch.float32, torch.float16):
        raise RuntimeError("linear_f32: out_dtype must be fp32 or fp16")
    epi = _EPILOGUES[epilogue]
    Nout = N // 2 if epi == LINEAR_GEGLU else N
    if bias is not None:
        bias = bias.detach().float().contiguous()
    for t, name in ((rows, "rows"), (rows2, "rows2")):
        if t is not None:
            _req(t, name)
    n_pad = (n + pad_to - 1) // pad_to * pad_to
    if out is None:
        out = torch.empty((B, Nout, n_pad) if transposed else (B, n_pad, Nout), dtype=out_dtype, device=x0.device)
        if n_pad != n:
            (out[:, :, n:] if transposed else out[:, n:]).zero_()
    if out.stride(2) != 1 or out.dtype != out_dtype:
        raise RuntimeError("linear_f32: out must be of out_dtype and contiguous along its last axis")
    if epi == LINEAR_RESID and (resid is None or resid.dtype != torch.float32 or resid.shape[0] != B
                                or resid.stride()[B == 1:] != out.stride()[B == 1:]):
        raise RuntimeError("linear_f32: resid must be fp32 with the strides of the result")
    _check(lib().vtm_linear_f32(_ptr(x0), P0, _ptr(x1), P1, B, K, _ptr(rows), 0 if rows is None else rows.shape[1],
                                _ptr(rows2), n, _ptr(weight), _ptr(bias), N, epi, _ptr(resid), out.data_ptr(),
                                dtype_code(out), out.stride(1), out.stride(0), int(transposed), _stream()),
           "vtm_linear_f32")
    return out


# ---- panel GEMMs (csrc/ff.hip): the feed-forward and the cross-attention query projection of the patched block ----
def panel_rows(n: int) -> int:
    return (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD


@_on_device
def to_panels(x: torch.Tensor, order: Optional[torch.Tensor] = None, rows: Optional[int] = None) -> torch.Tensor:
    """(rows, C) row-major -> k-panels (C / 8, rows_pad, 8); ``order`` (n,) int32: output row r = x[order[r]] (-1 = zeros)."""
    _req(x, "x")
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    n = x2.shape[0] if order is None else order.numel()
    n = n if rows is None else rows
    out = torch.empty((C // 8, panel_rows(n), 8), dtype=x.dtype, device=x.device)
    _check(lib().vtm_to_panels(_ptr(x2), dtype_code(x2), n, C, _ptr(order), _ptr(out), out.shape[1], _stream()),
           "vtm_to_panels")
    return out


@_on_device
def layernorm_panels(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    """torch.nn.LayerNorm over the last axis, result as k-panels (C / 8, rows_pad, 8) (rows = all leading axes flattened)."""
    _req(x, "x")
    C = x.shape[-1]
    xc = x.contiguous()
    rows = xc.numel() // C
    out = torch.empty((C // 8, panel_rows(rows), 8), dtype=x.dtype, device=x.device)
    _check(lib().vtm_layernorm_panels(_ptr(xc), _ptr(weight), _ptr(bias), dtype_code(xc), rows, C, float(eps), _ptr(out),
                                      out.shape[1], _stream()), "vtm_layernorm_panels")
    return out


@_on_device
def layernorm_gather(x: torch.Tensor, rows: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                     eps: float, panels: bool = True) -> torch.Tensor:
    """torch.nn.LayerNorm of x[b, rows[b, i], :] (x (B, L, C), rows (B, n) int32 with every entry in [0, L): not checked on the
    device), as k-panels (C / 8, panel_rows(B n), 8) with sample b at rows b * n, or (``panels=False``) as (B, n, C) token rows.
    Every row is bit-equal to that row of layernorm_panels / layernorm over x (vtm_layernorm_gather, include/vidtome_hip.h)."""
    _req(x, "x"), _req(rows, "rows")
    if x.dim() != 3 or rows.dim() != 2 or rows.shape[0] != x.shape[0] or rows.dtype != torch.int32 or rows.device != x.device:
        raise RuntimeError("vidtome_amd: layernorm_gather takes x (B, L, C) and rows (B, n) int32 on x's device")
    B, L, C = x.shape
    n = rows.shape[1]
    for name, p in (("weight", weight), ("bias", bias)):
        if p is not None and (p.dtype != x.dtype or p.numel() != C or p.device != x.device):
            raise RuntimeError(f"vidtome_amd: layernorm_gather {name} must be a ({C},) {x.dtype} tensor on {x.device}")
    if panels:
        out = torch.empty((C // 8, panel_rows(B * n), 8), dtype=x.dtype, device=x.device)
    else:
        out = torch.empty((B, n, C), dtype=x.dtype, device=x.device)
    _check(lib().vtm_layernorm_gather(_ptr(x), _ptr(weight.contiguous() if weight is not None else None),
                                      _ptr(bias.contiguous() if bias is not None else None), dtype_code(x), B, L, C, _ptr(rows), n,
                                      float(eps), _ptr(out), out.shape[1] if panels else 0, _stream()), "vtm_layernorm_gather")
    return out


@_on_device
def ff_geglu(x_panels: torch.Tensor, n: int, w1_panels: torch.Tensor, D: int, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """value * gelu(gate) of the GEGLU projection, panels in, panels (D / 8, n_pad, 8) out; see include/vidtome_hip.h."""
    K = x_panels.shape[0] * 8
    out = torch.empty((D // 8, x_panels.shape[1], 8), dtype=x_panels.dtype, device=x_panels.device)
    _check(lib().vtm_ff_geglu(_ptr(x_panels), n, x_panels.shape[1], _ptr(w1_panels), D, w1_panels.shape[1], K, _ptr(bias),
                              dtype_code(x_panels), _ptr(out), _stream()), "vtm_ff_geglu")
    return out


@_on_device
def linear_panels(x_panels: torch.Tensor, n: int, w_panels: torch.Tensor, N: int, bias: Optional[torch.Tensor],
                  resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n, N) token rows = x W^T (+ bias) (+ resid), panels in; see include/vidtome_hip.h.  Either operand may be a row
    range of a larger panel tensor (a view ``p[:, r0:r1]``: the panel stride is taken from the view); ``out`` may be a
    preallocated (n, N) view with a row stride >= N."""
    K = x_panels.shape[0] * 8
    if x_panels.stride(2) != 1 or x_panels.stride(1) != 8 or w_panels.stride(2) != 1 or w_panels.stride(1) != 8 \
            or w_panels.shape[0] * 8 != K:
        raise RuntimeError("linear_panels: operands must be (K / 8, rows, 8) panel tensors (or row ranges of one)")
    if out is None:
        out = torch.empty((n, N), dtype=x_panels.dtype, device=x_panels.device)
    if out.stride(1) != 1 or out.shape[0] < n or out.shape[1] < N:
        raise RuntimeError("linear_panels: out must be an (n, N) view, contiguous along its rows")
    if resid is not None:
        _req(resid, "resid")
        if resid.numel() != n * N or resid.dtype != out.dtype or out.stride(0) != N:
            raise RuntimeError("linear_panels: residual shape / dtype mismatch")
    _check(lib().vtm_linear_panels(_ptr(x_panels), n, x_panels.stride(0) // 8, _ptr(w_panels), N, w_panels.stride(0) // 8, K,
                                   _ptr(bias), _ptr(resid), dtype_code(x_panels), out.data_ptr(), out.stride(0), _stream()),
           "vtm_linear_panels")
    return out


# ---- attention broadcast (csrc/broadcast.hip): a segment's per-frame residual delta, recorded and replayed ----
def _broadcast_operands(who: str, h: torch.Tensor, caches, frame_ids: Optional[torch.Tensor]):
    """(G, Fg, num_frames, E) of a group-major batch ``h`` (G Fg, ...) against whole-video caches (G, num_frames, ...) of the
    same trailing shape, dtype and device.  ``frame_ids``: None (the chunk is frames 0 .. Fg - 1 = the whole video) or a device
    int32 (Fg,) tensor of distinct ids in [0, num_frames) -- NOT checked, here or on the device: the caller validates them."""
    _req(h, "h")
    first = caches[0]
    for c in caches:
        _req(c, "cache")
        if c.dim() < 3 or c.shape != first.shape or c.dtype != h.dtype or c.device != h.device or c.shape[2:] != h.shape[1:]:
            raise RuntimeError(f"{who}: a cache must be (G, num_frames, {', '.join(map(str, h.shape[1:]))}) {h.dtype} on "
                               f"{h.device}, got {tuple(c.shape)} {c.dtype} on {c.device}")
    G, num_frames = first.shape[:2]
    if frame_ids is None:
        Fg = num_frames
    else:
        if not frame_ids.is_cuda or frame_ids.device != h.device or frame_ids.dtype != torch.int32 or frame_ids.dim() != 1 \
                or not frame_ids.is_contiguous():
            raise RuntimeError(f"{who}: frame_ids must be a contiguous 1-D int32 tensor on {h.device}")
        Fg = frame_ids.numel()
    if h.dim() < 2 or not 1 <= Fg <= num_frames or h.shape[0] != G * Fg:
        raise RuntimeError(f"{who}: the batch has {h.shape[0]} samples, the caches hold G = {G} groups and the call carries "
                           f"Fg = {Fg} of {num_frames} frames (G Fg samples, group-major)")
    return G, Fg, num_frames, h[0].numel()


@_on_device
def residual_record(h_in: torch.Tensor, h_out: torch.Tensor, cache: torch.Tensor,
                    frame_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cache[g, id(f)] = (h_out.float() - h_in.float()).to(dtype)[g * Fg + f]: vtm_residual_record (include/vidtome_hip.h).
    Cache rows the ids do not name are left as they are.  Returns ``cache``."""
    who = "residual_record"
    G, Fg, num_frames, E = _broadcast_operands(who, h_in, (cache,), frame_ids)
    _req(h_out, "h_out")
    if h_out.shape != h_in.shape or h_out.dtype != h_in.dtype or h_out.device != h_in.device:
        raise RuntimeError(f"{who}: h_out must be like h_in")
    _check(lib().vtm_residual_record(_ptr(h_in), _ptr(h_out), _ptr(cache), _ptr(frame_ids), dtype_code(h_in), G, Fg, num_frames,
                                     E, _stream()), "vtm_residual_record")
    return cache


@_on_device
def residual_replay(h: torch.Tensor, cache1: torch.Tensor, cache2: Optional[torch.Tensor] = None,
                    frame_ids: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(h.float() + cache1[g, id(f)].float()).to(dtype), then the same with ``cache2`` on the rounded sum: vtm_residual_replay.
    ``out`` may be ``h``."""
    who = "residual_replay"
    G, Fg, num_frames, E = _broadcast_operands(who, h, (cache1,) if cache2 is None else (cache1, cache2), frame_ids)
    if out is None:
        out = torch.empty_like(h)
    elif out.shape != h.shape or out.dtype != h.dtype or out.device != h.device or not out.is_contiguous():
        raise RuntimeError(f"{who}: out must be like h")
    _check(lib().vtm_residual_replay(_ptr(h), _ptr(cache1), _ptr(cache2), _ptr(frame_ids), dtype_code(h), G, Fg, num_frames, E,
                                     _ptr(out), _stream()), "vtm_residual_replay")
    return out


@_on_device
def residual_replay_layernorm(h: torch.Tensor, cache1: torch.Tensor, cache2: Optional[torch.Tensor],
                              frame_ids: Optional[torch.Tensor], weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                              eps: float, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``residual_replay`` of h (G Fg, N, C) to token rows and, in the same launch, the LayerNorm of those rows as k-panels
    (C / 8, panel_rows(G Fg N), 8), every written row bit-equal to ``layernorm_panels`` of the rows: (rows, panels).
    fp16 / bf16, C a multiple of 64, at most 2048 (vtm_residual_replay_layernorm)."""
    who = "residual_replay_layernorm"
    if h.dim() != 3:
        raise RuntimeError(f"{who}: h must be (G Fg, N, C)")
    G, Fg, num_frames, _ = _broadcast_operands(who, h, (cache1,) if cache2 is None else (cache1, cache2), frame_ids)
    _, N, C = h.shape
    for name, p in (("weight", weight), ("bias", bias)):
        if p is not None and (p.dtype != h.dtype or p.numel() != C or p.device != h.device or not p.is_contiguous()):
            raise RuntimeError(f"{who}: {name} must be a contiguous ({C},) {h.dtype} tensor on {h.device}")
    if out is None:
        out = torch.empty_like(h)
    elif out.shape != h.shape or out.dtype != h.dtype or out.device != h.device or not out.is_contiguous():
        raise RuntimeError(f"{who}: out must be like h")
    panels = torch.empty((C // 8, panel_rows(G * Fg * N), 8), dtype=h.dtype, device=h.device)
    _check(lib().vtm_residual_replay_layernorm(_ptr(h), _ptr(cache1), _ptr(cache2), _ptr(frame_ids), _ptr(weight), _ptr(bias),
                                               float(eps), dtype_code(h), G, Fg, num_frames, N, C, _ptr(out), _ptr(panels),
                                               panels.shape[1], _stream()), "vtm_residual_replay_layernorm")
    return out, panels


@_on_device
def gather_panels(x0: torch.Tensor, x1: Optional[torch.Tensor], rows: Optional[torch.Tensor], rows2: Optional[torch.Tensor],
                  n: int) -> torch.Tensor:
    """Panels (C / 8, B * n_pad, 8) of pool[b, rows[b, rows2[b, i]]], i < n, sample b at rows b * n_pad (n_pad = n rounded up
    to 256, padding rows zero); pool = x0 | x1 as for gather_rows."""
    _req(x0, "x0")
    B, P0, C = x0.shape
    P1 = 0 if x1 is None else _req(x1, "x1").shape[1]
    n_pad = panel_rows(n)
    out = torch.empty((C // 8, B * n_pad, 8), dtype=x0.dtype, device=x0.device)
    _check(lib().vtm_gather_panels(_ptr(x0), P0, _ptr(x1), P1, dtype_code(x0), B, C, _ptr(rows),
                                   0 if rows is None else rows.shape[1], _ptr(rows2), n, _ptr(out), n_pad, _stream()),
           "vtm_gather_panels")
    return out


@_on_device
def lora_fold(w: torch.Tensor, up: torch.Tensor, down: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W + up @ down in w's dtype (fp32 accumulation, one rounding): w (c_out, c_in), up (c_out, r) and down (r, c_in) fp32;
    see include/vidtome_hip.h vtm_lora_fold."""
    _req(w, "w"), _req(up, "up"), _req(down, "down")
    c_out, c_in = w.shape
    r = up.shape[1]
    if up.dtype != torch.float32 or down.dtype != torch.float32 or tuple(up.shape) != (c_out, r) \
            or tuple(down.shape) != (r, c_in) or up.device != w.device or down.device != w.device:
        raise RuntimeError("lora_fold: up must be (c_out, r) and down (r, c_in) fp32 tensors on w's device")
    if out is None:
        out = torch.empty_like(w)
    _check(lib().vtm_lora_fold(_ptr(w), dtype_code(w), _ptr(up), _ptr(down), c_out, c_in, r, _ptr(_req(out, "out")),
                               _stream()), "vtm_lora_fold")
    return out


def _fold_operands(what: str, w: torch.Tensor, up: torch.Tensor, down: torch.Tensor, k_dora: int) -> Tuple[int, int, int]:
    _req(w, "w"), _req(up, "up"), _req(down, "down")
    c_out, c_in = w.shape
    r = up.shape[1]
    if up.dtype != torch.float32 or down.dtype != torch.float32 or tuple(up.shape) != (c_out, r) \
            or tuple(down.shape) != (r, c_in) or up.device != w.device or down.device != w.device:
        raise RuntimeError(f"{what}: up must be (c_out, r) and down (r, c_in) fp32 tensors on w's device")
    if not 0 < k_dora <= r:
        raise RuntimeError(f"{what}: k_dora {k_dora} not in [1, r = {r}]")
    return c_out, c_in, r


@_on_device
def dora_norms(w: torch.Tensor, up: torch.Tensor, down: torch.Tensor, k_dora: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 (c_out,) row norms of W + up[:, :k_dora] @ down[:k_dora] (operands as for lora_fold); see
    include/vidtome_hip.h vtm_dora_norms."""
    c_out, c_in, r = _fold_operands("dora_norms", w, up, down, k_dora)
    if out is None:
        out = torch.empty(c_out, dtype=torch.float32, device=w.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (c_out,) or out.device != w.device:
        raise RuntimeError("dora_norms: out must be an fp32 (c_out,) tensor on w's device")
    _check(lib().vtm_dora_norms(_ptr(w), dtype_code(w), _ptr(up), _ptr(down), c_out, c_in, r, k_dora, _ptr(_req(out, "out")),
                                _stream()), "vtm_dora_norms")
    return out


@_on_device
def dora_fold(w: torch.Tensor, up: torch.Tensor, down: torch.Tensor, magnitude: torch.Tensor, k_dora: int,
              norms: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(magnitude / norms) (W + up[:, :k_dora] @ down[:k_dora]) + up[:, k_dora:] @ down[k_dora:] in w's dtype, row-scaled,
    for a layer whose first adapter is DoRA: the DoRA adapter's columns / rows first in up / down (operands as for
    lora_fold), magnitude fp32 (c_out,); `norms` = dora_norms(w, up, down, k_dora) unless given.  See
    include/vidtome_hip.h vtm_dora_fold."""
    c_out, c_in, r = _fold_operands("dora_fold", w, up, down, k_dora)
    if norms is None:
        norms = dora_norms(w, up, down, k_dora)
    for name, t in (("magnitude", magnitude), ("norms", norms)):
        if t.dtype != torch.float32 or tuple(t.shape) != (c_out,) or t.device != w.device:
            raise RuntimeError(f"dora_fold: {name} must be an fp32 (c_out,) tensor on w's device")
    if out is None:
        out = torch.empty_like(w)
    _check(lib().vtm_dora_fold(_ptr(w), dtype_code(w), _ptr(up), _ptr(down), _ptr(_req(magnitude, "magnitude")),
                               _ptr(_req(norms, "norms")), c_out, c_in, r, k_dora, _ptr(_req(out, "out")), _stream()),
           "vtm_dora_fold")
    return out


def _f32_matrix(what: str, name: str, t: torch.Tensor, device) -> torch.Tensor:
    _req(t, name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.device != device:
        raise RuntimeError(f"{what}: {name} must be an fp32 matrix on the operands' device")
    return t


def _delta_out(what: str, out: Optional[torch.Tensor], accumulate: bool, c_out: int, c_in: int, device) -> torch.Tensor:
    if out is None:
        if accumulate:
            raise RuntimeError(f"{what}: accumulate needs the delta to add to (out)")
        return torch.empty((c_out, c_in), dtype=torch.float32, device=device)
    if tuple(_f32_matrix(what, "out", out, device).shape) != (c_out, c_in):
        raise RuntimeError(f"{what}: out must be ({c_out}, {c_in})")
    return out


@_on_device
def loha_delta(w1a: torch.Tensor, w1b: torch.Tensor, w2a: torch.Tensor, w2b: torch.Tensor,
               out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """fp32 (c_out, c_in) delta of one LoHa adapter, (w1a @ w1b) * (w2a @ w2b) elementwise (the adapter's scale already in
    w1a): written to `out` (a new tensor when None) or, with ``accumulate``, added to it; see include/vidtome_hip.h
    vtm_loha_delta."""
    dev = w1a.device
    for name, t in (("w1a", w1a), ("w1b", w1b), ("w2a", w2a), ("w2b", w2b)):
        _f32_matrix("loha_delta", name, t, dev)
    (c_out, r), c_in = w1a.shape, w1b.shape[1]
    if tuple(w1b.shape) != (r, c_in) or tuple(w2a.shape) != (c_out, r) or tuple(w2b.shape) != (r, c_in):
        raise RuntimeError("loha_delta: w1a / w2a must be (c_out, r) and w1b / w2b (r, c_in) with one rank r")
    out = _delta_out("loha_delta", out, accumulate, c_out, c_in, dev)
    _check(lib().vtm_loha_delta(_ptr(w1a), _ptr(w1b), _ptr(w2a), _ptr(w2b), c_out, c_in, r, int(bool(accumulate)), _ptr(out),
                                _stream()), "vtm_loha_delta")
    return out


@_on_device
def lokr_delta(w1: torch.Tensor, w2: torch.Tensor, out: Optional[torch.Tensor] = None,
               accumulate: bool = False) -> torch.Tensor:
    """fp32 (a1 a2, b1 b2) delta of one LoKr adapter, kron(w1 (a1, b1), w2 (a2, b2)) (the adapter's scale already in w1):
    written to `out` or, with ``accumulate``, added to it; see include/vidtome_hip.h vtm_lokr_delta."""
    dev = w1.device
    _f32_matrix("lokr_delta", "w1", w1, dev), _f32_matrix("lokr_delta", "w2", w2, dev)
    (a1, b1), (a2, b2) = w1.shape, w2.shape
    out = _delta_out("lokr_delta", out, accumulate, a1 * a2, b1 * b2, dev)
    _check(lib().vtm_lokr_delta(_ptr(w1), _ptr(w2), a1, b1, a2, b2, a1 * a2, b1 * b2, int(bool(accumulate)), _ptr(out),
                                _stream()), "vtm_lokr_delta")
    return out


@_on_device
def delta_fold(w: torch.Tensor, delta: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32(w) + delta rounded once to w's dtype: w (c_out, c_in), delta fp32 of the same shape; see
    include/vidtome_hip.h vtm_delta_fold."""
    _req(w, "w")
    if w.dim() != 2 or tuple(_f32_matrix("delta_fold", "delta", delta, w.device).shape) != tuple(w.shape):
        raise RuntimeError("delta_fold: delta must be an fp32 tensor of w's (c_out, c_in) shape on its device")
    if out is None:
        out = torch.empty_like(w)
    if out.dtype != w.dtype or tuple(out.shape) != tuple(w.shape) or out.device != w.device:
        raise RuntimeError("delta_fold: out must have w's shape, dtype and device")
    c_out, c_in = w.shape
    _check(lib().vtm_delta_fold(_ptr(w), dtype_code(w), _ptr(delta), c_out, c_in, _ptr(_req(out, "out")), _stream()),
           "vtm_delta_fold")
    return out
