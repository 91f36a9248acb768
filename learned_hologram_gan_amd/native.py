"""ctypes binding of liblhg_hip.so (C ABI: include/lhg_hip.h).

The product path has no CPU or eager-PyTorch fallback: if the library is missing, fails to load
or lacks a symbol, ``load()`` raises.  Every wrapper passes raw device pointers and PyTorch's
current HIP stream, and turns a non-zero status into ``RuntimeError(lhg_last_error())``.
"""

from __future__ import annotations

import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblhg_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lhg_hip.h")

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3
IN_POLAR, IN_PHASE, IN_COMPLEX = 0, 1, 2
OUT_COMPLEX, OUT_ABS_ANGLE, OUT_ABS = 0, 1, 2
F_NONE, F_MUL, F_MUL_CONJ, F_DIV, F_DIV_CONJ = 0, 1, 2, 3, 4

_p, _i, _f, _ll, _sz = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_size_t


class AsmFilter(C.Structure):
    _fields_ = [("f1", _p), ("f1_index", _p), ("f1_op", _i), ("f2", _p), ("f2_index", _p), ("f2_op", _i)]


class PackItem(C.Structure):
    """lhg_pack_item (include/lhg_hip.h)."""
    _fields_ = [("w", C.c_void_p), ("dst", C.c_void_p), ("D0", C.c_int), ("D1", C.c_int), ("KH", C.c_int), ("KW", C.c_int),
                ("rows_from_d0", C.c_int), ("rows_pad", C.c_int), ("k_pad", C.c_int)]


# name -> argtypes (restype is int unless listed in _RESTYPE)
ABI_VERSION = 10  # LHG_ABI_VERSION of include/lhg_hip.h this binding was written against

_SIGNATURES = {
    "lhg_abi_version": [],
    "lhg_last_error": [],
    "lhg_autotune": [_i],
    "lhg_profile_enable": [_i, _i],
    "lhg_profile_read": [_i, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)],
    "lhg_nchw_to_nhwc": [_p, _p, _i, _i, _i, _i, _i, _p],
    "lhg_nhwc_to_nchw": [_p, _i, _p, _i, _i, _i, _i, _p],
    "lhg_set_conv_precision": [_i],
    "lhg_get_conv_precision": [],
    "lhg_set_activation_dtype": [_i],
    "lhg_get_activation_dtype": [],
    "lhg_default_conv_precision": [],
    "lhg_packed_weight_floats": [C.c_int, C.c_int, C.c_int],
    "lhg_pack_weight": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _p],
    "lhg_pack_weights": [_p, _i, _p],
    "lhg_conv2d_forward": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _i, _i, _f, _i, _p, _p, _p],
    "lhg_conv2d_stats_rows_bound": [_i, _i, _i],
    "lhg_conv2d_forward_thin_res": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _i, _p, _p, _i, _f, _p, _p, _p],
    "lhg_gather_gemm_splitk_floats": [_ll, _ll, _i, _i, _i],
    "lhg_gather_gemm_workspace": [_p, _ll],
    "lhg_conv2d_forward_stats": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, C.POINTER(C.c_int), _p],
    "lhg_bn_stats_finish": [_p, _i, _p, _ll, _i, _p, _p, _p, _f, _f, _p],
    "lhg_conv2d_backward_input": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _p, _i, _i, _p, _p],
    "lhg_conv2d_backward_input_add": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _p, _i, _i, _p, _i, _p, _p],
    "lhg_conv2d_backward_input_add_amax": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _p, _i, _i, _p, _i, _p, _p, _p],
    "lhg_conv_transpose2x2_backward_input_amax": [_p, _i, _i, _i, _i, _i, _p, _i, _p, _i, _i, _p, _p, _p],
    "lhg_conv2d_wgrad_splits": [_i, _i, _i, _i, _i, _i, _i, _i],
    "lhg_conv2d_backward_weight": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _p, _p, _p],
    "lhg_conv2d_thin_supported": [_i, _i, _i, _i],
    "lhg_conv2d_thin_forward": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _p, _i, _p, _p, _p, _i, _f, _i, _p],
    "lhg_conv2d_thin_forward_amax": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _p, _i, _p, _p, _p, _i, _f, _i, _p, _p],
    "lhg_conv2d_thin_forward_nchw": [_p, _i, _i, _i, _i, _p, _i, _i, _p, _i, _p, _p, _p, _i, _f, _p, _p],
    "lhg_conv2d_thin_backward_input": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _p, _i, _p],
    "lhg_conv2d_thin_wgrad_workspace": [_i, _i, _i, _i, _i, _i],
    "lhg_conv2d_thin_backward_weight": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _p, _p, _sz, _p],
    "lhg_conv_transpose2x2_forward": [_p, _i, _i, _i, _i, _i, _p, _i, _p, _i, _i, _p, _p, _p, _p],
    "lhg_conv_transpose2x2_backward_input": [_p, _i, _i, _i, _i, _i, _p, _i, _p, _i, _i, _p, _p],
    "lhg_conv_transpose2x2_wgrad_splits": [_i, _i, _i, _i, _i],
    "lhg_conv_transpose2x2_backward_weight": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _p, _i, _i, _i, _p, _p, _p],
    "lhg_absmax": [_p, _ll, _i, _i, _p, _p],
    "lhg_channel_absmax": [_p, _ll, _i, _i, _p, _p, _p],
    "lhg_chanmax_partial_rows": [_ll, _i],
    "lhg_channel_absmax_finish": [_p, _ll, _i, _p, _p],
    "lhg_channel_absmax_finish_rows": [_p, _i, _i, _p, _p],
    "lhg_bn_apply_chanmax": [_p, _i, _ll, _i, _p, _p, _p, _p, _i, _i, _f, _p, _i, _p, _p, _p],
    "lhg_bn_backward_chanmax": [_p, _i, _p, _i, _p, _i, _ll, _i, _p, _p, _i, _f, _p, _i, _p, _i, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p],
    "lhg_wgrad_reduce": [_p, _i, _i, _i, _i, _p, _i, _i, _i, _i, _p],
    "lhg_channel_sum": [_p, _ll, _i, _i, _p, _i, _p, _p],
    "lhg_bn_stats": [_p, _ll, _i, _i, _p, _p, _p, _f, _f, _p, _p],
    "lhg_bn_apply": [_p, _i, _ll, _i, _p, _p, _p, _p, _i, _i, _f, _p, _i, _p, _p],
    "lhg_bn_backward": [_p, _i, _p, _i, _p, _i, _ll, _i, _p, _p, _i, _f, _p, _i, _p, _i, _p, _p, _i, _p, _p, _p, _p],
    "lhg_bn_eval_backward": [_p, _i, _p, _i, _p, _i, _ll, _i, _p, _p, _i, _f, _p, _i, _p, _i, _p, _p, _p, _p, _p],
    "lhg_bn_backward_backward": [_p, _p, _p, _p, _ll, _i, _p, _p, _i, _f, _p, _p, _p, _p, _p],
    "lhg_bn_backward_sums": [_p, _i, _p, _i, _p, _i, _ll, _i, _p, _p, _i, _f, _p, _p, _p, _p],
    "lhg_bn_backward_apply": [_p, _i, _p, _i, _p, _i, _ll, _i, _p, _p, _p, _f, _i, _f, _p, _i, _p, _i, _p, _p, _p],
    "lhg_bn_backward_backward_sums": [_p, _p, _p, _p, _ll, _i, _p, _p, _i, _f, _p, _p, _p],
    "lhg_bn_backward_backward_apply": [_p, _p, _p, _p, _ll, _i, _p, _p, _p, _f, _i, _f, _p, _p, _p, _p],
    "lhg_maxpool2x2_forward": [_p, _i, _i, _i, _i, _i, _p, _i, _p],
    "lhg_maxpool2x2_backward": [_p, _i, _p, _i, _i, _i, _i, _i, _p, _i, _p],
    "lhg_maxpool2x2_backward_add": [_p, _i, _p, _i, _i, _i, _i, _i, _p, _i, _p, _i, _p],
    "lhg_act_backward": [_p, _i, _p, _i, _ll, _i, _i, _f, _p, _i, _p],
    "lhg_asm_propagate": [_p, _p, _i, _f, _i, _i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _sz, _p, _p, _p],
    "lhg_asm_propagate_shared": [_p, _p, _i, _f, _i, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _sz, _p, _p, _p],
    "lhg_asm_to_spectrum": [_p, _p, _i, _f, _i, _i, _i, _i, _i, _p, _p, _p, _sz, _p, _p, _p],
    "lhg_asm_from_spectrum": [_p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _sz, _p, _p, _p],
    "lhg_asm_from_spectrum_shared": [_p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _sz, _p, _p, _p],
    "lhg_fft_table_floats": [_i],
    "lhg_fft_twiddles": [_p, _i, _p],
    "lhg_symconv_field": [_p, _i, _i, _i, _p, _p, _p, _p, _p],
    "lhg_double_phase_encode": [_p, _p, _i, _i, _i, _p, _p],
    "lhg_poh_partial_blocks": [_i, _i],
    "lhg_double_phase_encode_backward": [_p, _p, _p, _i, _i, _i, _p, _p, _p],
    "lhg_symconv_field_backward": [_p, _p, _i, _i, _i, _p, _p, _p, _p],
    "lhg_polar_output_cotangent": [_p, _p, _p, _f, _p, _ll, _p],
    "lhg_polar_input_cotangent": [_p, _p, _p, _f, _f, _p, _p, _ll, _p],
    "lhg_recon_loss_blocks": [_i, _i, _i],
    "lhg_recon_loss_forward": [_p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p],
    "lhg_recon_loss_backward": [_p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p],
    "lhg_psnr_ssim_workspace": [_i, _i, _i],
    "lhg_psnr_ssim": [_p, _p, _i, _i, _i, _p, _p, _sz, _p],
    "lhg_adam_step": [_p, _p, _p, _p, _ll, _f, _f, _f, _f, _i, _p],
    "lhg_adam_step_scaled": [_p, _p, _p, _p, _ll, _f, _f, _f, _f, _i, _f, _p, _p],
    "lhg_conv2d_backward_weight_workspace": [_i, _i, _i, _i, _i, _i, _i, _i],
    "lhg_conv2d_backward_weight_into": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _i, _p, _i, _p, _sz, _p, _p, _p],
    "lhg_conv_transpose2x2_backward_weight_workspace": [_i, _i, _i, _i, _i],
    "lhg_conv_transpose2x2_backward_weight_into": [_p, _i, _i, _i, _i, _i, _p, _i, _i, _p, _i, _p, _sz, _p, _p, _p],
    "lhg_fused_workspace_floats": [],
    "lhg_fused_ticket_count": [],
    "lhg_bn_forward_train": [_p, _i, _ll, _i, _p, _p, _p, _p, _f, _f, _p, _i, _i, _f, _p, _i, _p, _p, _p, _i, _p, _p, _p],
    "lhg_bn_backward_fused": [_p, _i, _p, _i, _p, _i, _ll, _i, _p, _p, _p, _i, _f, _p, _i, _p, _i, _p, _p, _i, _p, _p, _p, _p, _i, _p, _p, _p],
    "lhg_bn_backward_backward_fused": [_p, _p, _p, _p, _ll, _i, _p, _p, _i, _f, _p, _p, _p, _p, _p, _p],
    "lhg_channel_sum_fused": [_p, _ll, _i, _i, _p, _i, _p, _p, _p],
    "lhg_channel_absmax_fused": [_p, _ll, _i, _i, _p, _p, _p, _p],
    "lhg_wg6_force": [_i, _i, _i],
    "lhg_wg6_last_plan": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "lhg_wg6_variants": [],
    "lhg_wg6_variant_name": [_i],
}
_RESTYPE = {"lhg_last_error": C.c_char_p, "lhg_fused_workspace_floats": C.c_longlong, "lhg_packed_weight_floats": C.c_longlong, "lhg_fft_table_floats": C.c_longlong, "lhg_chanmax_partial_rows": C.c_longlong, "lhg_conv2d_stats_rows_bound": C.c_longlong, "lhg_gather_gemm_splitk_floats": C.c_longlong, "lhg_conv2d_thin_wgrad_workspace": C.c_size_t, "lhg_psnr_ssim_workspace": C.c_size_t,
            "lhg_conv2d_backward_weight_workspace": C.c_size_t, "lhg_conv_transpose2x2_backward_weight_workspace": C.c_size_t, "lhg_wg6_variant_name": C.c_char_p}

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def declared_symbols(header_path: str = HEADER_PATH):
    """Function names declared in include/lhg_hip.h (used by the CPU test that checks that the
    library exports exactly the declared ABI)."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lhg_[a-z0-9_]+)\s*\(", text)))


def load():
    """Load the gfx950 library; raises NativeLibraryError when it cannot be used."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950). There is no CPU / eager fallback for the hot path."
        )
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, argtypes in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
        fn.argtypes = argtypes
        fn.restype = _RESTYPE.get(name, C.c_int)
    prio = os.environ.get("LHG_GG_PRIO")
    if prio is not None and prio.strip() not in ("0", "1", "2"):
        # values >= 10 used to select timing ablations of the gather-GEMM that gave WRONG results on purpose (rounds 2 - 4); they are gone
        # from the kernels, and a stale environment must not pass silently: the C side refuses the launch as well (conv_engine.hip)
        raise NativeLibraryError(f"LHG_GG_PRIO={prio!r}: only 0, 1, 2 exist (s_setprio placement; the wrong-result timing ablations were removed)")
    got = lib.lhg_abi_version()
    if got != ABI_VERSION:
        raise NativeLibraryError(f"ABI version mismatch: library {got}, binding {ABI_VERSION}")
    _lib = lib
    return lib


# torch.cuda.current_stream() builds a Stream object per call (~9 us; ~500 calls per train step: 4 - 5 ms of the host's launch loop,
# tools/host_profile.py); the raw getters behind it return the same hipStream_t in well under a microsecond.
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_RAW_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr() -> int:
    """The current HIP stream of the current device as an integer handle (what every lhg_* entry point takes last)."""
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return _RAW_STREAM(_RAW_DEVICE())
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise NativeLibraryError("HIP op called with a CPU tensor: the hot path runs on the GPU only (no CPU fallback)")
    return t.data_ptr()


def call(name: str, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.lhg_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{name} failed ({rc}): {msg}")


class kernel_profile:
    """Context manager: time every gather-GEMM (0) / wgrad-GEMM (1) launch with HIP events and count the
    ALGORITHMIC flops (true channel counts, no padding) the Python op layer attributes to them."""

    algorithmic = [0.0, 0.0]
    active = False

    def __enter__(self):
        for k in (0, 1):
            call("lhg_profile_enable", k, 1)
        kernel_profile.algorithmic = [0.0, 0.0]
        kernel_profile.active = True
        return self

    def __exit__(self, *exc):
        kernel_profile.active = False
        self.result = []
        for k in (0, 1):
            ms, n, fl = C.c_double(), C.c_longlong(), C.c_double()
            call("lhg_profile_read", k, C.byref(ms), C.byref(n), C.byref(fl))
            call("lhg_profile_enable", k, 0)
            self.result.append(dict(total_ms=ms.value, launches=n.value, executed_flops=fl.value,
                                    algorithmic_flops=kernel_profile.algorithmic[k]))
        return False


def count_flops(kernel: int, flops: float):
    if kernel_profile.active:
        kernel_profile.algorithmic[kernel] += flops
