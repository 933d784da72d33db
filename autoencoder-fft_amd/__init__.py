"""ctypes binding of libaefft.so (include/aefft.h) -- plumbing for tests and bench.py.

The product is the HIP library; this module only moves pointers.  torch provides device
memory (tensor.data_ptr()), the stream and torch.distributed; no arithmetic happens here.
There is NO CPU fallback: importing succeeds without the library only so that CPU-side tests
can inspect the host logic, but every compute call raises if libaefft.so or the GPU is missing.

Import with:  aefft = importlib.import_module("autoencoder-fft_amd")
"""
import atexit
import ctypes as C
import os
import math

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (AEFFT_LIB: development only -- tools/x*.sh point the binding at an experiment build under build_x/ instead of copying it over the product)
LIB_PATH = os.environ.get("AEFFT_LIB") or os.path.join(_HERE, "libaefft.so")

OK, EINVAL, EHIP, ENOMEM, ESTATE = 0, 1, 2, 3, 4


# include/aefft.h AEFFT_F_* (development switches; tests/test_abi.py checks this table against the header)
FLAGS = {n: 1 << i for i, n in enumerate(
    ["NOLAZY", "NOCOMPACT", "NOQPATH", "NOFUSEMSE", "NOGROUP", "NOMFMA", "NOGFWD", "NOOVERLAP", "NOFUSECROP", "GTAPS",
     "NOPREFETCH", "NODEFER", "NOTILEDSPATIAL", "NOFAST", "NOSPLITK", "POISON", "NOOPFORM", "NOCHAIN", "NOFUSEUPD", "NOAHEAD", "NORCORR", "NOLAZYMSE", "SMALLOVERLAP", "CHAINMSE",
     "CHIRPZ", "NOPRUNESMOOTH", "NOSTATICCHAIN"])}
NET_SMOOTH_SIZES = 1 << 0   # include/aefft.h AEFFT_NET_SMOOTH_SIZES (aefft_net_create_ex)
NET_SPATIAL = 1 << 1        # include/aefft.h AEFFT_NET_SPATIAL: the coordinate-space training mode as a resident net
NET_SMOOTH_OPFORM = 1 << 2  # include/aefft.h AEFFT_NET_SMOOTH_OPFORM: the operator-form training step on grids with a smooth axis


class AefftError(RuntimeError):
    pass


class NetDesc(C.Structure):
    _fields_ = [("D", C.c_int), ("Nx", C.c_int), ("Ny", C.c_int), ("npairs", C.c_int),
                ("maps", C.POINTER(C.c_int)), ("Nk", C.POINTER(C.c_int)), ("Nl", C.POINTER(C.c_int)),
                ("scale", C.POINTER(C.c_int)), ("batch", C.c_int)]


class YuvDesc(C.Structure):
    """include/aefft.h aefft_yuv_desc"""
    _fields_ = [("format", C.c_int), ("matrix", C.c_int), ("W", C.c_int), ("H", C.c_int),
                ("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("stride", C.c_size_t * 3)]


class YuvDst(C.Structure):
    """include/aefft.h aefft_yuv_dst"""
    _fields_ = [("format", C.c_int), ("matrix", C.c_int), ("W", C.c_int), ("H", C.c_int),
                ("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("stride", C.c_size_t * 3)]


class RawDesc(C.Structure):
    """include/aefft.h aefft_raw_desc"""
    _fields_ = [("pattern", C.c_int), ("container", C.c_int), ("bits", C.c_int), ("W", C.c_int), ("H", C.c_int),
                ("data", C.c_void_p), ("pitch", C.c_size_t), ("stride", C.c_size_t), ("black", C.c_int), ("white", C.c_int),
                ("gain", C.c_float * 3), ("method", C.c_int), ("ccm", C.POINTER(C.c_float)), ("lut_d", C.c_void_p)]


class TileDesc(C.Structure):
    """include/aefft.h aefft_tile_desc"""
    _fields_ = [("W", C.c_int), ("H", C.c_int), ("Nx", C.c_int), ("Ny", C.c_int),
                ("overlap_x", C.c_int), ("overlap_y", C.c_int), ("rim_x", C.c_int), ("rim_y", C.c_int)]


class TilePlan(C.Structure):
    """include/aefft.h aefft_tile_plan"""
    _fields_ = [("ntx", C.c_int), ("nty", C.c_int), ("ox0", C.c_int), ("oy0", C.c_int),
                ("step_x", C.c_int), ("step_y", C.c_int), ("ramp_x", C.c_int), ("ramp_y", C.c_int)]


class Region(C.Structure):
    """include/aefft.h aefft_region (32 bytes; REGION is the numpy form)"""
    _fields_ = [("i0", C.c_int), ("j0", C.c_int), ("i1", C.c_int), ("j1", C.c_int), ("area", C.c_int), ("peak_i", C.c_int), ("peak_j", C.c_int),
                ("peak", C.c_float)]


class Affine(C.Structure):
    """include/aefft.h aefft_affine: six Q24 coefficients of the row-major 2 x 3 matrix (48 bytes)"""
    _fields_ = [("a", C.c_longlong * 6)]


class Shift(C.Structure):
    """include/aefft.h aefft_shift: the estimated shift of one image (16 bytes; SHIFT is the numpy form)"""
    _fields_ = [("dx", C.c_float), ("dy", C.c_float), ("response", C.c_float), ("cell", C.c_int)]


_lib = None
_vp, _fp, _i, _l, _f = C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_float   # device float* passed as void*

# name -> (restype, argtypes); must list every symbol declared in include/aefft.h
SIGNATURES = {
    "aefft_ctx_create": (_i, [C.POINTER(_vp), _i, _vp, _i]),
    "aefft_ctx_destroy": (None, [_vp]),
    "aefft_last_error": (C.c_char_p, [_vp]),
    "aefft_sync": (_i, [_vp]),
    "aefft_ctx_partition": (_i, [_vp, _i]),
    "aefft_ctx_set_flags": (_i, [_vp, C.c_uint]),
    "aefft_ctx_get_flags": (C.c_uint, [_vp]),
    "aefft_stream": (_vp, [_vp]),
    "aefft_version": (C.c_char_p, []),
    "aefft_r2c": (_i, [_vp, _fp, _fp, _l, _i, _i]),
    "aefft_c2r": (_i, [_vp, _fp, _fp, _l, _i, _i, _f]),
    "aefft_pool": (_i, [_vp, _fp, _fp, _l, _i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "aefft_r2c_pool": (_i, [_vp, _fp, _fp, _l, _i, _i, _i]),
    "aefft_unpool_c2r": (_i, [_vp, _fp, _fp, _l, _i, _i, _i, _f]),
    "aefft_kernel_spectrum": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _i, _i]),
    "aefft_kernel_export": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _i, _i]),
    "aefft_conv": (_i, [_vp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i]),
    "aefft_gradient": (_i, [_vp] + [_fp] * 10 + [_i] * 5),
    "aefft_mse": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i]),
    "aefft_update": (_i, [_vp] + [_fp] * 14 + [_i] * 6 + [_f, _i]),
    "aefft_conv_spatial": (_i, [_vp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i]),
    "aefft_pool_spatial": (_i, [_vp, _fp, _fp, C.c_long, _i, _i, _i, _i, _i]),
    "aefft_pool_conv_spatial": (_i, [_vp, _fp, _fp, _fp, _fp, _fp] + [_i] * 9),
    "aefft_backprop_spatial": (_i, [_vp] + [_fp] * 15 + [_i] * 7 + [_f, _f, _i, _i]),
    "aefft_step_spatial": (_i, [_vp] + [_fp] * 15 + [_i] * 7 + [_f, _f, _i, _i]),
    "aefft_image_to_frames": (_i, [_vp, _vp, C.c_size_t, _vp, _i, _i, _i, _i, _i]),
    "aefft_frames_to_image": (_i, [_vp, _vp, _i, _vp, C.c_size_t, _i, _i, _i, _i]),
    "aefft_image_resize_to_frames": (_i, [_vp, _vp, C.c_size_t, C.c_size_t, _i, _i, _i, _vp, _i, _i, _i, _i, _i]),
    "aefft_frames_resize_to_image": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, C.c_size_t, C.c_size_t, _i, _i, _i, _i]),
    "aefft_map_overlay_image": (_i, [_vp, _fp, _i, _i, _f, _f, _i, _vp, _i, _vp, C.c_size_t, C.c_size_t, _i, _i, _i, _i]),
    "aefft_frames_degrade": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _f, C.c_ulonglong, C.c_ulonglong]),
    "aefft_yuv_to_image": (_i, [_vp, C.POINTER(YuvDesc), _i, _vp, C.c_size_t, C.c_size_t, _i]),
    "aefft_yuv_resize_to_frames": (_i, [_vp, C.POINTER(YuvDesc), _i, _i, _vp, _i, _i, _i, _i]),
    "aefft_tile_plan_make": (_i, [C.POINTER(TileDesc), C.POINTER(TilePlan)]),
    "aefft_image_tiles_to_frames": (_i, [_vp, _vp, C.c_size_t, C.c_size_t, C.POINTER(TileDesc), _vp, _i, _i, _i]),
    "aefft_frames_tiles_to_image": (_i, [_vp, _vp, _i, C.POINTER(TileDesc), _vp, C.c_size_t, C.c_size_t, _i, _i]),
    "aefft_image_to_yuv": (_i, [_vp, _vp, C.c_size_t, C.c_size_t, _i, C.POINTER(YuvDst), _i]),
    "aefft_frames_resize_to_yuv": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.POINTER(YuvDst), _i]),
    "aefft_image_compare_map": (_i, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _i, _i, _i, _i, _i, _i, _i, _fp, _fp]),
    "aefft_map_regions_workspace": (C.c_size_t, [_i, _i, _i]),
    "aefft_map_regions": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _f, _f, _i, _i, _vp, _vp, _i, _vp, _vp, C.c_size_t]),
    "aefft_region_to_pixels": (_i, [C.POINTER(Region), _i, _i, _i, _i] + [C.POINTER(_i)] * 4),
    "aefft_raw_to_image": (_i, [_vp, C.POINTER(RawDesc), _i, _vp, C.c_size_t, C.c_size_t, _i]),
    "aefft_map_stats_bytes": (C.c_size_t, [_i, _i]),
    "aefft_map_stats_update": (_i, [_vp, _fp, _i, _i, _i, _vp, C.c_size_t]),
    "aefft_map_stats_merge": (_i, [_vp, _vp, _vp, _i, _i, C.c_size_t]),
    "aefft_map_stats_finish": (_i, [_vp, _vp, C.c_size_t, _i, _i, _i, _i, _f, _i, _f, _fp]),
    "aefft_map_peak": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _fp, _vp]),
    "aefft_affine_make": (_i, [C.POINTER(C.c_double), C.POINTER(Affine)]),
    "aefft_image_warp_affine": (_i, [_vp, _vp, C.c_size_t, C.c_size_t, _i, _i, _vp, _i, _i, _i, C.c_uint, _vp, C.c_size_t, C.c_size_t, _i, _i, _i, _i]),
    "aefft_image_remap": (_i, [_vp, _vp, C.c_size_t, C.c_size_t, _i, _i, _vp, _i, _i, C.c_uint, _vp, C.c_size_t, C.c_size_t, _i, _i, _i, _i]),
    "aefft_register_spec_floats": (C.c_size_t, [_i, _i]),
    "aefft_register_workspace": (C.c_size_t, [_i, _i, _i]),
    "aefft_frames_register_ref": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _fp, _vp, C.c_size_t]),
    "aefft_frames_register": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _fp, _i, _f, _f, C.c_double, C.c_double, _vp, _vp, _vp, C.c_size_t]),
    "aefft_net_create": (_i, [_vp, C.POINTER(NetDesc), C.POINTER(_vp)]),
    "aefft_net_create_ex": (_i, [_vp, C.POINTER(NetDesc), C.c_uint, C.POINTER(_vp)]),
    "aefft_net_destroy": (None, [_vp]),
    "aefft_net_npairs": (_i, [_vp]),
    "aefft_net_pair_shape": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "aefft_net_set_pair": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "aefft_net_get_pair": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "aefft_net_pair_spectra": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp)]),
    "aefft_net_load_spectra": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "aefft_net_store_spectra": (_i, [_vp, _i, _vp, _vp]),
    "aefft_net_forward": (_i, [_vp, _fp, _fp]),
    "aefft_net_get_layer": (_i, [_vp, _i, _fp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "aefft_net_layers_layout": (_i, [_vp, C.POINTER(C.c_size_t)]),
    "aefft_net_get_layers": (_i, [_vp, _fp]),
    "aefft_magnitude": (_i, [_vp, _fp, _fp, _l, _i, _i, _i, _i]),
    "aefft_net_train_pair": (_i, [_vp, _i, _i, _f, _i, _i, _vp]),
    "aefft_net_step_grad": (_i, [_vp, _fp, _fp]),
    "aefft_net_step_grad_u8": (_i, [_vp, _vp, _fp]),
    "aefft_net_step_grad_target": (_i, [_vp, _vp, _i, _vp, _i, _fp]),
    "aefft_net_forward_u8": (_i, [_vp, _vp, _fp]),
    "aefft_net_infer": (_i, [_vp, _vp, _i, _vp, _i, _i, _fp]),
    "aefft_net_decode": (_i, [_vp, _i, _fp, _vp, _i]),
    "aefft_net_score": (_i, [_vp, _vp, _i, _fp, _fp]),
    "aefft_net_score_map": (_i, [_vp, _vp, _i, _i, _fp, _fp, _fp]),
    "aefft_net_score_target": (_i, [_vp, _vp, _i, _vp, _i, _fp, _fp]),
    "aefft_net_score_map_target": (_i, [_vp, _vp, _i, _vp, _i, _i, _fp, _fp, _fp]),
    "aefft_net_ssim_map": (_i, [_vp, _vp, _i, _vp, _i, _i, _f, _fp, _fp, _fp]),
    "aefft_net_set_input_ready": (_i, [_vp, _i]),
    "aefft_net_grad_buffer": (_i, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "aefft_net_step_form": (_i, [_vp]),
    "aefft_net_tail_route": (_i, [_vp]),
    "aefft_net_last_mse": (_i, [_vp, _vp]),
    "aefft_net_step_apply": (_i, [_vp, _f, _i, _i, _f, _fp]),
    "aefft_net_reset_momentum": (_i, [_vp]),
    "aefft_net_set_inertia": (_i, [_vp, _f]),
    "aefft_prof_enable": (_i, [_vp, _i]),
    "aefft_prof_count": (_i, []),
    "aefft_prof_name": (C.c_char_p, [_i]),
    "aefft_prof_read": (_i, [_vp, _i, C.POINTER(_l), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "aefft_prof_reset": (_i, [_vp]),
}


def lib():
    """Load libaefft.so and declare every prototype; raises if the HIP library was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AefftError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


DP_LIB_PATH = os.path.join(_HERE, "libaefft_dp.so")
_dp_lib = None
# include/aefft_dp.h (libaefft_dp.so = libaefft.so + librccl): name -> (restype, argtypes)
DP_SIGNATURES = {
    "aefft_dp_unique_id": (_i, [_vp]),
    "aefft_dp_create": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(_vp)]),
    "aefft_dp_destroy": (None, [_vp]),
    "aefft_dp_last_error": (C.c_char_p, [_vp]),
    "aefft_dp_step": (_i, [_vp, _fp, _fp, _f, _i, _i, _fp]),
    "aefft_dp_run": (_i, [_vp, _fp, _fp, _f, _i, _i, _i]),
    "aefft_dp_profile": (_i, [_vp, _fp, _fp, _f, _i, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "aefft_dp_flush_mse": (_i, [_vp, _vp]),
    "aefft_dp_allreduce_bytes": (C.c_size_t, [_vp]),
    "aefft_dp_replicas_agree": (_i, [_vp]),
}
DP_ID_BYTES = 128


def dp_lib():
    """Load libaefft_dp.so (the data-parallel step over RCCL, include/aefft_dp.h); raises if it was not built."""
    global _dp_lib
    if _dp_lib is None:
        lib()                                             # libaefft.so first: the same image the nets were created from
        if not os.path.exists(DP_LIB_PATH):
            raise AefftError(f"{DP_LIB_PATH} not built: run `make -C autoencoder-fft_amd/csrc dp` (__graft_entry__.build does)")
        L = C.CDLL(DP_LIB_PATH)
        for name, (res, args) in DP_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _dp_lib = L
    return _dp_lib


_exiting = False


def _mark_exit():
    global _exiting
    _exiting = True


atexit.register(_mark_exit)


def _ptr(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def _is_u8(t):
    import torch
    return t is not None and t.dtype == torch.uint8


def _hptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _image_layout(image, what):
    """(the image as [B][Ny][Nx][D], pitch in bytes) of a uint8 tensor [B][Ny][Nx][D] or [Ny][Nx][D] of interleaved image rows: contiguous, or a
    row-padded view -- stride(-1) == 1, stride(-2) == D, stride(-3) = pitch >= Nx * D and, for a batch, stride(0) == Ny * pitch"""
    if image.dtype != torch.uint8 or image.dim() not in (3, 4):
        raise ValueError(f"{what}: the image must be a uint8 tensor [B][Ny][Nx][D] or [Ny][Nx][D]")
    try:
        img, pitch, stride = _resize_layout(image, what)
        if img.shape[0] > 1 and img.shape[1] > 1 and stride != img.shape[1] * pitch:
            raise ValueError
    except ValueError:
        raise ValueError(f"{what}: the image must be contiguous or a row-padded view (stride(-1) == 1, stride(-2) == D, stride(-3) = pitch >= Nx * D, "
                         f"stride(0) == Ny * pitch); got shape {tuple(image.shape)} with strides {tuple(image.stride())}") from None
    return img, stride if img.shape[1] == 1 else pitch       # (one row an image: the batch stride is the pitch)


RESIZE_MODES = {"linear": 0, "area": 1}      # AEFFT_RESIZE_LINEAR, AEFFT_RESIZE_AREA
YUV_FORMATS = {"nv12": 0, "i420": 1, "yuyv": 2}      # AEFFT_YUV_NV12, AEFFT_YUV_I420, AEFFT_YUV_YUYV
YUV_MATRICES = {"bt601": 0, "bt709": 1, "jpeg": 2}   # AEFFT_YUV_BT601, AEFFT_YUV_BT709, AEFFT_YUV_JPEG
YUV_ORDERS = {"bgr": 0, "rgb": 1, "gray": 2}         # AEFFT_YUV_BGR, AEFFT_YUV_RGB, AEFFT_YUV_GRAY: D = 3, 3, 1


def _resize_layout(image, what):
    """(the image as [B][H][W][D], pitch, image stride in bytes) of a uint8 tensor [B][H][W][D] or [H][W][D] of interleaved image rows as
    aefft_image_resize_to_frames takes them: stride(-1) == 1, stride(-2) == D, stride(-3) = pitch >= W * D and ANY batch stride of at least
    (H - 1) * pitch + W * D -- contiguous, row-padded, or a region of interest big[:, y0:y1, x0:x1] of a larger batch"""
    if image.dtype != torch.uint8 or image.dim() not in (3, 4):
        raise ValueError(f"{what}: the image must be a uint8 tensor [B][H][W][D] or [H][W][D]")
    img = image if image.dim() == 4 else image.unsqueeze(0)
    B, H, W, D = img.shape
    sb, sy, sx, sd = img.stride()
    if min(B, H, W, D) < 1:
        raise ValueError(f"{what}: empty image of shape {tuple(image.shape)}")
    pitch = sy if H > 1 else W * D
    extent = (H - 1) * pitch + W * D
    if (D > 1 and sd != 1) or (W > 1 and sx != D) or pitch < W * D or (B > 1 and sb < extent):
        raise ValueError(f"{what}: the image must have stride(-1) == 1, stride(-2) == D, stride(-3) = pitch >= W * D and a batch stride of at least "
                         f"(H - 1) * pitch + W * D; got shape {tuple(image.shape)} with strides {tuple(image.stride())}")
    return img, int(pitch), int(sb if B > 1 else extent)


def _yuv_source(planes, fmt, matrix, order, what):
    """the checks of the YUV calls that need no device: (the filled YuvDesc, B, W, H, D, the plane tensors the descriptor points into).  `planes`
    is a tuple of uint8 tensors -- nv12 (y [B][H][W], uv [B][Hc][Wc][2]), i420 (y, u [B][Hc][Wc], v), yuyv (yuyv [B][H][W/2][4],), or the same
    without the batch axis -- each contiguous or a view with stride(-1) == 1 (the interleaved axes whole), a row pitch and any sufficient batch
    stride, checked like _resize_layout: two views into one decoder surface therefore work.  With order "gray" only the luma plane is looked at."""
    if fmt not in YUV_FORMATS or matrix not in YUV_MATRICES or order not in YUV_ORDERS:
        raise ValueError(f"{what}: fmt must be one of {sorted(YUV_FORMATS)}, matrix of {sorted(YUV_MATRICES)}, order of {sorted(YUV_ORDERS)}")
    try:
        planes = tuple(planes)
    except TypeError:
        raise ValueError(f"{what}: planes must be a tuple of uint8 tensors") from None
    need = {"nv12": 2, "i420": 3, "yuyv": 1}[fmt]
    used = 1 if order == "gray" else need
    if len(planes) not in (need, used) or any(p is None for p in planes[:used]):
        raise ValueError(f"{what}: {fmt} takes {need} plane(s)")
    inner = {"nv12": (1, 2), "i420": (1, 1, 1), "yuyv": (4,)}[fmt]      # interleaved bytes per element of a plane's row
    views, desc = [], YuvDesc()
    desc.format, desc.matrix = YUV_FORMATS[fmt], YUV_MATRICES[matrix]
    B = W = H = None
    for k, p in enumerate(planes[:used]):
        rank = 3 if inner[k] == 1 else 4
        if not isinstance(p, torch.Tensor) or p.dtype != torch.uint8 or p.dim() not in (rank - 1, rank):
            raise ValueError(f"{what}: plane {k} must be a uint8 tensor with {rank} axes (or {rank - 1}, unbatched)")
        v = p if p.dim() == rank else p.unsqueeze(0)
        v = v if rank == 4 else v.unsqueeze(-1)
        img, pitch, stride = _resize_layout(v, f"{what}: plane {k}")
        b, rows, cols, e = img.shape
        if e != inner[k]:
            raise ValueError(f"{what}: plane {k} must have {inner[k]} interleaved bytes per element, got {e}")
        if k == 0:
            B, H, W = b, rows, cols * (2 if fmt == "yuyv" else 1)
        elif (b, rows, cols) != (B, (H + 1) // 2, (W + 1) // 2):
            raise ValueError(f"{what}: plane {k} must be {(B, (H + 1) // 2, (W + 1) // 2)} chroma samples for a luma plane of {(B, H, W)}, got {(b, rows, cols)}")
        views.append(img)
        desc.plane[k], desc.pitch[k], desc.stride[k] = img.data_ptr(), pitch, stride
    if W > 8192 or H > 8192:
        raise ValueError(f"{what}: W, H must be in 1..8192")
    desc.W, desc.H = W, H
    return desc, B, W, H, 1 if order == "gray" else 3, views


def yuv_plane_shapes(fmt, B, W, H):
    """the shapes of the plane tensors of B images of W x H luma samples, as yuv_to_image takes and image_to_yuv returns them"""
    Wc, Hc = (W + 1) // 2, (H + 1) // 2
    return {"nv12": [(B, H, W), (B, Hc, Wc, 2)], "i420": [(B, H, W), (B, Hc, Wc), (B, Hc, Wc)], "yuyv": [(B, H, W // 2, 4)]}[fmt]


def _yuv_dest(fmt, matrix, order, B, W, H, D, out, what):
    """the checks of the calls that WRITE YUV planes that need no device: fmt, matrix and order are known names, the source has the channels the
    order names (D), W is even for yuyv, and `out` -- None, or the tuple of uint8 plane tensors to fill, laid out as _yuv_source takes them and of
    yuv_plane_shapes(fmt, B, W, H) -- fits.  Returns the filled YuvDst (None without `out`) and the views it points into."""
    if fmt not in YUV_FORMATS or matrix not in YUV_MATRICES or order not in YUV_ORDERS:
        raise ValueError(f"{what}: fmt must be one of {sorted(YUV_FORMATS)}, matrix of {sorted(YUV_MATRICES)}, order of {sorted(YUV_ORDERS)}")
    if D != (1 if order == "gray" else 3):
        raise ValueError(f"{what}: order {order!r} names {1 if order == 'gray' else 3} channel(s), the source has {D}")
    if min(W, H) < 1 or W > 8192 or H > 8192:
        raise ValueError(f"{what}: W, H must be in 1..8192")
    if fmt == "yuyv" and W % 2:
        raise ValueError(f"{what}: yuyv needs an even W")
    if out is None:
        return None, []
    src, b, w, h, _, views = _yuv_source(out, fmt, matrix, "bgr", f"{what}: out")      # (every plane of the format, whatever the order)
    if (b, w, h) != (B, W, H):
        raise ValueError(f"{what}: out must be the planes of {B} images of {W} x {H}: shapes {yuv_plane_shapes(fmt, B, W, H)}")
    dst = YuvDst()
    dst.format, dst.matrix, dst.W, dst.H = src.format, src.matrix, W, H
    for k in range(3):
        dst.plane[k], dst.pitch[k], dst.stride[k] = src.plane[k], src.pitch[k], src.stride[k]
    return dst, views


RAW_PATTERNS = {"rggb": 0, "grbg": 1, "gbrg": 2, "bggr": 3, "mono": 4}      # AEFFT_RAW_RGGB .. AEFFT_RAW_MONO: GenICam's names (BayerRG = "rggb")
RAW_CONTAINERS = {"u8": 0, "u16": 1, "packed": 2}                            # AEFFT_RAW_U8, AEFFT_RAW_U16, AEFFT_RAW_PACKED
DEMOSAIC_METHODS = {"bilinear": 0, "mhc": 1}                                 # AEFFT_DEMOSAIC_BILINEAR, AEFFT_DEMOSAIC_MHC


def _raw_source(raw, pattern, bits, packed, black, white, gains, method, order, ccm, what):
    """the checks of Context.raw_to_image that need no device: (the filled RawDesc without its table, B, W, H, D, what the descriptor points
    into).  `raw` is a uint8 tensor [B][H][bytes] or [H][bytes] -- bits == 8: one sample a byte; packed: GenICam 10p / 12p rows, the last axis
    the row's ceil(W * bits / 8) bytes, so W = 8 * bytes // bits -- or an int16 / uint16 tensor [B][H][W] or [H][W] with the sample in the low
    `bits` bits; contiguous, or a view with stride(-1) == 1, a row pitch and any sufficient batch stride."""
    import torch
    if pattern not in RAW_PATTERNS or method not in DEMOSAIC_METHODS or (pattern != "mono" and order not in ("bgr", "rgb")):
        raise ValueError(f"{what}: pattern must be one of {sorted(RAW_PATTERNS)}, method of {sorted(DEMOSAIC_METHODS)}, order 'bgr' or 'rgb'")
    words = tuple(getattr(torch, n) for n in ("int16", "uint16") if hasattr(torch, n))
    if not isinstance(raw, torch.Tensor) or raw.dtype not in (torch.uint8,) + words or raw.dim() not in (2, 3):
        raise ValueError(f"{what}: raw must be a uint8, int16 or uint16 tensor [B][H][W] or [H][W] (uint8 packed: the rows' bytes)")
    bits = int(bits)
    if raw.dtype == torch.uint8:
        container = "packed" if packed else "u8"
        if (packed and bits not in (10, 12)) or (not packed and bits != 8):
            raise ValueError(f"{what}: a uint8 tensor holds 8-bit samples, or with packed=True 10- or 12-bit ones")
    else:
        container = "u16"
        if packed or not 9 <= bits <= 16:
            raise ValueError(f"{what}: a 16-bit tensor holds samples of 9..16 bits, not packed")
    v = raw if raw.dim() == 3 else raw.unsqueeze(0)
    B, H, cols = v.shape
    es = v.element_size()
    sb, sy, sx = v.stride()
    if min(B, H, cols) < 1 or (cols > 1 and sx != 1):
        raise ValueError(f"{what}: raw must be non-empty with stride(-1) == 1; got shape {tuple(raw.shape)} with strides {tuple(raw.stride())}")
    W = 8 * cols // bits if packed else cols
    live = cols * es
    pitch = sy * es if H > 1 else live
    extent = (H - 1) * pitch + live
    stride = sb * es if B > 1 else extent
    if pitch < live or stride < extent:
        raise ValueError(f"{what}: rows or images of raw overlap; got shape {tuple(raw.shape)} with strides {tuple(raw.stride())}")
    if not (4 <= W <= 8192 and 4 <= H <= 8192):
        raise ValueError(f"{what}: W, H must be in 4..8192, got {(W, H)}")
    white = (1 << bits) - 1 if white is None else int(white)
    black = int(black)
    if not 0 <= black < white <= (1 << bits) - 1:
        raise ValueError(f"{what}: black and white must satisfy 0 <= black < white <= 2^bits - 1")
    mono = pattern == "mono"
    try:
        g = [float(x) for x in ([gains] if isinstance(gains, (int, float)) else gains)]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: gains must be three numbers (R, G, B), or one for mono") from None
    if len(g) not in ((1, 3) if mono else (3,)) or not all(np.isfinite(x) and 0.0 <= x <= 64.0 for x in g):
        raise ValueError(f"{what}: gains must be three finite numbers (R, G, B) in 0..64, or one for mono")
    desc = RawDesc()
    desc.pattern, desc.container, desc.bits, desc.W, desc.H = RAW_PATTERNS[pattern], RAW_CONTAINERS[container], bits, W, H
    desc.data, desc.pitch, desc.stride, desc.black, desc.white = v.data_ptr(), pitch, stride, black, white
    for k in range(3):
        desc.gain[k] = g[k if k < len(g) else 0]
    desc.method = DEMOSAIC_METHODS[method]
    keep = [v]
    if ccm is not None and not mono:
        m = np.asarray(ccm, dtype=np.float32).reshape(-1)
        if m.size != 9 or not np.isfinite(m).all() or (np.abs(m) >= 4).any():
            raise ValueError(f"{what}: ccm must be 9 finite numbers (3 x 3, row-major, out = ccm * (R, G, B)) below 4 in magnitude")
        arr = (C.c_float * 9)(*m.tolist())
        desc.ccm = C.cast(arr, C.POINTER(C.c_float))
        keep.append(arr)
    return desc, B, W, H, 1 if mono else 3, keep


def gamma_lut(gamma=2.2):
    """The 4096-byte table of Context.raw_to_image for a power law, as a numpy uint8 array: entry k stands for the linear value k / 16 grey
    levels, lut[k] = floor(255 * (min(k, 4080) / 4080) ** (1 / gamma) + 0.5) in double; entries above 4080 (never read) repeat 255."""
    gamma = float(gamma)
    if not np.isfinite(gamma) or gamma <= 0:
        raise ValueError("gamma_lut: gamma must be finite and positive")
    x = np.minimum(np.arange(4096, dtype=np.float64), 4080.0) / 4080.0
    return np.floor(255.0 * x ** (1.0 / gamma) + 0.5).astype(np.uint8)


def srgb_lut():
    """The 4096-byte table of Context.raw_to_image for the sRGB transfer curve (IEC 61966-2-1), as a numpy uint8 array: with
    x = min(k, 4080) / 4080, lut[k] = floor(255 * (12.92 x if x <= 0.0031308 else 1.055 x ** (1 / 2.4) - 0.055) + 0.5) in double."""
    x = np.minimum(np.arange(4096, dtype=np.float64), 4080.0) / 4080.0
    y = np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1.0 / 2.4) - 0.055)
    return np.floor(255.0 * y + 0.5).astype(np.uint8)


def heat_lut(D=3):
    """A default colour table for Context.map_overlay as a numpy uint8 [256][D], from integer formulas: entry k runs from blue (k = 0) through
    green to red (k = 255) in the image's own BGR order -- B = 255 - k, G = 255 - |2 k - 255|, R = k; D == 1 a grey ramp k; D == 2 (k, 255);
    D == 4 BGR with the fourth channel 255."""
    if D not in (1, 2, 3, 4):
        raise ValueError("heat_lut: D must be 1..4")
    k = np.arange(256, dtype=np.int64)
    if D == 1:
        cols = [k]
    elif D == 2:
        cols = [k, np.full(256, 255)]
    else:
        cols = [255 - k, 255 - np.abs(2 * k - 255), k] + ([np.full(256, 255)] if D == 4 else [])
    return np.ascontiguousarray(np.stack(cols, axis=1).astype(np.uint8))


def _frames4(frames, what, axes="[B][D][Nx][Ny]"):
    """the shape of frames as every boundary call takes them: contiguous, non-empty, uint8 or float32, four axes"""
    if frames.dtype not in (torch.uint8, torch.float32) or frames.dim() != 4 or not frames.is_contiguous() or min(frames.shape) < 1:
        raise ValueError(f"{what}: frames must be a contiguous, non-empty uint8 or float32 tensor {axes}")
    return frames.shape


def _two_ints(v, what, rule):
    """a size such as (W, H) as two ints; `rule` is the sentence for anything else"""
    try:
        x, y = (int(q) for q in v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {rule}") from None
    return x, y


def _frames_resize_args(frames, size, mode, out):
    """the checks of Context.frames_resize_to_image that need no device: (frames, (W, H), mode value); `out`, when given, is checked by the caller
    through _resize_layout"""
    what = "Context.frames_resize_to_image"
    B, D = _frames4(frames, what)[:2]
    if mode not in RESIZE_MODES:
        raise ValueError(f"{what}: mode must be one of {sorted(RESIZE_MODES)}")
    W, H = _two_ints(size, what, "size must be (W, H)")
    if W < 1 or H < 1:
        raise ValueError(f"{what}: size must be positive")
    if out is not None and (out.dim() != 4 or tuple(out.shape) != (B, H, W, D)):
        raise ValueError(f"{what}: out must be a uint8 tensor of shape {(B, H, W, D)}")
    return W, H, RESIZE_MODES[mode]


def _overlay_args(map, image, lut, lo, hi, alpha):
    """the checks of Context.map_overlay that need no device: (map as [B][Mx][My], image as [B][H][W][D], pitch, image stride)"""
    what = "Context.map_overlay"
    img, pitch, stride = _resize_layout(image, what)
    B, H, W, D = img.shape
    if map.dtype != torch.float32 or map.dim() not in (2, 3) or not map.is_contiguous() or min(map.shape) < 1:
        raise ValueError(f"{what}: map must be a contiguous, non-empty float32 tensor [B][Mx][My] or [Mx][My]")
    m = map if map.dim() == 3 else map.unsqueeze(0)
    if m.shape[0] != B:
        raise ValueError(f"{what}: map has {m.shape[0]} entries along the batch, the image {B}")
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, D) or not lut.is_contiguous():
        raise ValueError(f"{what}: lut must be a contiguous uint8 tensor of shape {(256, D)}")
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo == hi:
        raise ValueError(f"{what}: lo and hi must be finite and different")
    if int(alpha) != alpha or not 0 <= alpha <= 256:
        raise ValueError(f"{what}: alpha must be an integer in 0..256")
    return m, img, pitch, stride


def _frames_degrade_args(frames, blur, sigma, impulse, seed, first_frame, out, dtype):
    """the checks of Context.frames_degrade that need no device: (blur, sigma, impulse, seed, first_frame, the result's dtype) as the C call takes
    them; `out`, when given, has the frames' shape and is `frames` itself only in the element-wise case (blur == 0, the same dtype)"""
    what = "Context.frames_degrade"
    B, D, Nx, Ny = _frames4(frames, what)
    if not 1 <= D <= 4 or Nx > 8192 or Ny > 8192:
        raise ValueError(f"{what}: D must be 1..4 and Nx, Ny in 1..8192; got shape {tuple(frames.shape)}")
    if isinstance(blur, bool) or int(blur) != blur or not 0 <= blur <= 4:
        raise ValueError(f"{what}: blur must be an integer in 0..4")
    if not np.isfinite(sigma) or not 0 <= sigma <= 255:
        raise ValueError(f"{what}: sigma must be finite and in 0..255")
    if not np.isfinite(impulse) or not 0 <= impulse <= 1:
        raise ValueError(f"{what}: impulse must be finite and in 0..1")
    for name, v in (("seed", seed), ("first_frame", first_frame)):
        if isinstance(v, bool) or int(v) != v or not 0 <= v < 2 ** 64:
            raise ValueError(f"{what}: {name} must be an integer in 0..2^64 - 1")
    if out is not None:
        if dtype is not None and dtype != out.dtype:
            raise ValueError(f"{what}: dtype and out.dtype differ")
        dtype = out.dtype
    elif dtype is None:
        dtype = frames.dtype
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{what}: the result must be uint8 or float32")
    if out is not None:
        if tuple(out.shape) != tuple(frames.shape) or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous tensor of shape {tuple(frames.shape)}")
        if out.data_ptr() == frames.data_ptr() and (blur != 0 or out.dtype != frames.dtype):
            raise ValueError(f"{what}: in place (out=frames) needs blur == 0 and the frames' own dtype")
    return int(blur), float(sigma), float(impulse), int(seed), int(first_frame), dtype


def _pair(v, what, name):
    """an int, or an (x, y) pair of ints, as two ints"""
    try:
        x, y = (v, v) if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else v
        if any(isinstance(q, bool) or int(q) != q for q in (x, y)):
            raise TypeError
        return int(x), int(y)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be an int or an (x, y) pair of ints") from None


def tile_plan(W, H, Nx, Ny, overlap, rim=0):
    """The tile grid of tiled inference (aefft_tile_plan_make; host arithmetic, no device): an image of W x H pixels cut into tiles of Nx x Ny
    (Nx along the image's columns) that share `overlap` pixels with their neighbours, of which `rim` at each tile edge are never used.
    `overlap` and `rim` are each an int or an (x, y) pair.  Returns (the filled TileDesc, the TilePlan: ntx, nty, ox0, oy0, step_x, step_y,
    ramp_x, ramp_y); ValueError for what the library refuses (W, H in 1..8192; Nx, Ny in 2..2048; 0 <= 2 overlap <= N; 0 <= 2 rim <= overlap)."""
    what = "tile_plan"
    (vx, vy), (mx, my) = _pair(overlap, what, "overlap"), _pair(rim, what, "rim")
    try:
        desc = TileDesc(int(W), int(H), int(Nx), int(Ny), vx, vy, mx, my)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{what}: W, H, Nx, Ny must be ints") from None
    plan = TilePlan()
    if lib().aefft_tile_plan_make(C.byref(desc), C.byref(plan)) != 0:
        raise ValueError(f"{what}: W, H must be in 1..8192, Nx, Ny in 2..2048, 0 <= 2 overlap <= N and 0 <= 2 rim <= overlap per axis; got "
                         f"W={W} H={H} Nx={Nx} Ny={Ny} overlap={(vx, vy)} rim={(mx, my)}")
    return desc, plan


def _image_tiles_args(image, tile, overlap, rim, out, dtype):
    """the checks of Context.image_tiles_to_frames that need no device: (the image as [B][H][W][D], pitch, image stride, the TileDesc, the shape
    (T, D, Nx, Ny) of the tile frames, their dtype)"""
    what = "Context.image_tiles_to_frames"
    img, pitch, stride = _resize_layout(image, what)
    B, H, W, D = img.shape
    if not 1 <= D <= 4:
        raise ValueError(f"{what}: D must be 1..4")
    Nx, Ny = _two_ints(tile, what, "tile must be (Nx, Ny)")
    desc, plan = tile_plan(W, H, Nx, Ny, overlap, rim)
    shape = (B * plan.ntx * plan.nty, D, Nx, Ny)
    if out is not None:
        if out.dtype not in (torch.uint8, torch.float32) or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous uint8 or float32 tensor of shape {shape}")
        dtype = out.dtype
    elif dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{what}: dtype must be torch.uint8 or torch.float32")
    return img, pitch, stride, desc, shape, dtype


def _frames_tiles_args(frames, size, overlap, rim, out):
    """the checks of Context.frames_tiles_to_image that need no device: (the TileDesc, the shape (B, H, W, D) of the image); `out`, when given,
    is checked for that shape here and for its layout by the caller through _resize_layout"""
    what = "Context.frames_tiles_to_image"
    T, D, Nx, Ny = _frames4(frames, what, "[T][D][Nx][Ny]")
    if not 1 <= D <= 4:
        raise ValueError(f"{what}: D must be 1..4")
    W, H = _two_ints(size, what, "size must be (W, H)")
    desc, plan = tile_plan(W, H, Nx, Ny, overlap, rim)
    per = plan.ntx * plan.nty
    if T % per:
        raise ValueError(f"{what}: {T} frames are not a whole number of images of {plan.ntx} x {plan.nty} tiles")
    shape = (T // per, H, W, D)
    if out is not None and (out.dim() != 4 or tuple(out.shape) != shape):
        raise ValueError(f"{what}: out must be a uint8 tensor of shape {shape}")
    return desc, shape


COMPARE_METRICS = {"mse": 0, "ssim": 1}      # AEFFT_COMPARE_MSE, AEFFT_COMPARE_SSIM


def cells_for_tile(W, H, tile):
    """The cell grid (Mx, My) = (ceil(W / tx), ceil(H / ty)) that Context.image_compare_map takes for cells of about `tile` pixels a side on an
    image of W x H: `tile` is an int or an (x, y) pair in 1..64.  The cells are then floor(W / Mx) or ceil(W / Mx) <= tx columns wide."""
    what = "cells_for_tile"
    tx, ty = _pair(tile, what, "tile")
    try:
        W, H = int(W), int(H)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: W, H must be ints") from None
    if not (1 <= tx <= 64 and 1 <= ty <= 64) or W < 1 or H < 1:
        raise ValueError(f"{what}: tile must be in 1..64 per axis and W, H positive")
    return -(-W // tx), -(-H // ty)


def _image_compare_args(a, b, cells, metric, map, score):
    """the checks of Context.image_compare_map that need no device: (a as [B][H][W][D], its pitch and stride, b likewise, its pitch and stride,
    (Mx, My), the metric's value); `map` and `score`, when given, are checked for shape, dtype and layout"""
    what = "Context.image_compare_map"
    ia, pa, sa = _resize_layout(a, f"{what}: a")
    ib, pb, sb = _resize_layout(b, f"{what}: b")
    if tuple(ia.shape) != tuple(ib.shape):
        raise ValueError(f"{what}: a and b must have one shape; got {tuple(a.shape)} and {tuple(b.shape)}")
    B, H, W, D = ia.shape
    if not 1 <= D <= 4 or W > 8192 or H > 8192:
        raise ValueError(f"{what}: D must be 1..4 and W, H in 1..8192")
    if metric not in COMPARE_METRICS:
        raise ValueError(f"{what}: metric must be one of {sorted(COMPARE_METRICS)}")
    Mx, My = _two_ints(cells, what, "cells must be (Mx, My)")
    if not (1 <= Mx <= min(W, 1024) and 1 <= My <= min(H, 1024)) or -(-W // Mx) > 64 or -(-H // My) > 64:
        raise ValueError(f"{what}: cells must be 1 <= Mx <= min(W, 1024), 1 <= My <= min(H, 1024) with cells of at most 64 x 64 pixels; got "
                         f"{(Mx, My)} for an image of {W} x {H}")
    if map is not None and (map.dtype != torch.float32 or tuple(map.shape) != (B, Mx, My) or not map.is_contiguous()):
        raise ValueError(f"{what}: map must be a contiguous float32 tensor of shape {(B, Mx, My)}")
    if score is not None and score is not False and (score.dtype != torch.float32 or tuple(score.shape) != (B,) or not score.is_contiguous()):
        raise ValueError(f"{what}: score must be a contiguous float32 tensor of shape {(B,)}, None or False")
    return ia, pa, sa, ib, pb, sb, (Mx, My), COMPARE_METRICS[metric]


REGIONS_SENSE = {"above": 0, "below": 1}     # AEFFT_REGIONS_ABOVE, AEFFT_REGIONS_BELOW
# aefft_region as a numpy structured dtype: regions.cpu().numpy().view(REGION)[..., 0] of the int32 tensor [B][max_regions][8] Context.map_regions returns
REGION = np.dtype([("i0", "<i4"), ("j0", "<i4"), ("i1", "<i4"), ("j1", "<i4"), ("area", "<i4"), ("peak_i", "<i4"), ("peak_j", "<i4"), ("peak", "<f4")])


def _map_regions_args(map, lo, hi, ref, sense, connectivity, min_area, max_regions, labels, regions, count):
    """the checks of Context.map_regions that need no device: (map as [B][Mx][My], lo, hi, the sense's value, connectivity, min_area, max_regions);
    `ref`, `labels`, `regions` and `count`, when given, are checked for shape, dtype and layout"""
    what = "Context.map_regions"
    if map.dtype != torch.float32 or map.dim() not in (2, 3) or not map.is_contiguous():
        raise ValueError(f"{what}: map must be a contiguous float32 tensor [B][Mx][My] or [Mx][My]")
    m = map if map.dim() == 3 else map[None]
    B, Mx, My = m.shape
    if not (1 <= Mx <= 1024 and 1 <= My <= 1024 and B >= 1 and B * Mx * My <= 2 ** 31 - 1):
        raise ValueError(f"{what}: Mx, My must be in 1..1024, B >= 1 and B * Mx * My <= 2^31 - 1")
    if sense not in REGIONS_SENSE:
        raise ValueError(f"{what}: sense must be one of {sorted(REGIONS_SENSE)}")
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"{what}: connectivity must be 4 or 8")
    try:
        lo = float(lo)
        hi = lo if hi is None else float(hi)
        min_area, max_regions = int(min_area), int(max_regions)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: lo, hi must be numbers and min_area, max_regions ints") from None
    with np.errstate(over="ignore"):
        finite = bool(np.isfinite(np.float32(lo)) and np.isfinite(np.float32(hi)))         # (as floats: what the library receives)
    if not finite or (lo > hi if sense == "above" else hi > lo):
        raise ValueError(f"{what}: lo and hi must be finite, lo <= hi for sense='above' and hi <= lo for sense='below'")
    if min_area < 1 or not 0 <= max_regions <= 65536:
        raise ValueError(f"{what}: min_area must be >= 1 and max_regions in 0..65536")
    if ref is not None and (ref.dtype != torch.float32 or tuple(ref.shape) != (Mx, My) or not ref.is_contiguous()):
        raise ValueError(f"{what}: ref must be a contiguous float32 tensor of shape {(Mx, My)}")
    if labels is not None and (labels.dtype != torch.int32 or tuple(labels.shape) != (B, Mx, My) or not labels.is_contiguous()):
        raise ValueError(f"{what}: labels must be a contiguous int32 tensor of shape {(B, Mx, My)}")
    if regions is not None and (max_regions == 0 or regions.dtype != torch.int32 or tuple(regions.shape) != (B, max_regions, 8) or not regions.is_contiguous()):
        raise ValueError(f"{what}: regions must be a contiguous int32 tensor of shape {(B, max_regions, 8)} (None when max_regions == 0)")
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (B,) or not count.is_contiguous()):
        raise ValueError(f"{what}: count must be a contiguous int32 tensor of shape {(B,)}")
    return m, lo, hi, REGIONS_SENSE[sense], connectivity, min_area, max_regions


def region_pixels(region, cells, W, H):
    """The half-open pixel box (x0, y0, x1, y1) of a region on an image of W x H (aefft_region_to_pixels: Context.image_compare_map's cell rule,
    x0 = ceil(i0 W / Mx), x1 = ceil((i1 + 1) W / Mx), rows alike): `region` is one REGION record, a Region, or anything with i0, j0, i1, j1;
    cells = (Mx, My).  Host arithmetic; ValueError for bounds outside the grid or sizes outside image_compare_map's ranges."""
    Mx, My = _two_ints(cells, "region_pixels", "cells must be (Mx, My)")
    get = (lambda k: int(region[k])) if not isinstance(region, Region) else (lambda k: int(getattr(region, k)))
    r = Region(get("i0"), get("j0"), get("i1"), get("j1"), 0, 0, 0, 0.0)
    box = [C.c_int() for _ in range(4)]
    if lib().aefft_region_to_pixels(C.byref(r), Mx, My, int(W), int(H), *[C.byref(v) for v in box]) != OK:
        raise ValueError(f"region_pixels: bounds {(r.i0, r.j0, r.i1, r.j1)} outside the grid {(Mx, My)}, or W, H outside 1..8192, or more cells than pixels")
    return tuple(v.value for v in box)


CALIB_MODE = {"sigma": 0, "rank": 1}         # AEFFT_CALIB_SIGMA, AEFFT_CALIB_RANK


def map_stats_bytes(Mx, My):
    """aefft_map_stats_bytes without the library: 52 bytes a cell rounded up to a multiple of 16; 0 for sizes outside 1..1024"""
    return (52 * Mx * My + 15) // 16 * 16 if 1 <= Mx <= 1024 and 1 <= My <= 1024 else 0


def _stats_state(state, Mx, My, what, name="state"):
    """a calibration state of Mx x My cells: a contiguous 1-D uint8 tensor of at least map_stats_bytes(Mx, My) bytes"""
    need = map_stats_bytes(Mx, My)
    if not need:
        raise ValueError(f"{what}: Mx, My must be in 1..1024")
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or state.dim() != 1 or not state.is_contiguous() or state.numel() < need:
        raise ValueError(f"{what}: {name} must be a contiguous 1-D uint8 tensor of at least {need} bytes (Context.map_stats({Mx}, {My}))")
    return state


def map_stats_view(state, Mx, My):
    """The five planes of a calibration state as tensor views, in the layout include/aefft.h states: (S1, S2, hi, lo, c) with S1, S2 float64
    [Mx][My], hi, lo float32 [4][Mx][My] (hi[0] the largest, lo[0] the smallest; only the first min(c, 4) slots are live) and c int32 [Mx][My]."""
    Mx, My = _two_ints((Mx, My), "map_stats_view", "Mx, My must be ints")
    s = _stats_state(state, Mx, My, "map_stats_view")
    n = Mx * My
    return (s[:8 * n].view(torch.float64).view(Mx, My), s[8 * n:16 * n].view(torch.float64).view(Mx, My), s[16 * n:32 * n].view(torch.float32).view(4, Mx, My),
            s[32 * n:48 * n].view(torch.float32).view(4, Mx, My), s[48 * n:52 * n].view(torch.int32).view(Mx, My))


def _maps3(map, what):
    """a batch of maps as [B][Mx][My]"""
    if not isinstance(map, torch.Tensor) or map.dtype != torch.float32 or map.dim() not in (2, 3) or not map.is_contiguous():
        raise ValueError(f"{what}: map must be a contiguous float32 tensor [B][Mx][My] or [Mx][My]")
    m = map if map.dim() == 3 else map[None]
    B, Mx, My = m.shape
    if not (1 <= Mx <= 1024 and 1 <= My <= 1024 and B >= 1 and B * Mx * My <= 2 ** 31 - 1):
        raise ValueError(f"{what}: Mx, My must be in 1..1024, B >= 1 and B * Mx * My <= 2^31 - 1")
    return m


def _map_stats_update_args(state, map):
    """the checks of Context.map_stats_update that need no device: map as [B][Mx][My]"""
    what = "Context.map_stats_update"
    m = _maps3(map, what)
    _stats_state(state, m.shape[1], m.shape[2], what)
    return m


def _map_stats_merge_args(dst, src, cells):
    """the checks of Context.map_stats_merge that need no device: (Mx, My) -- `cells`, or what Context.map_stats noted on dst or src"""
    what = "Context.map_stats_merge"
    if cells is None:
        cells = getattr(dst, "cells", None) or getattr(src, "cells", None)
    if cells is None:
        raise ValueError(f"{what}: cells=(Mx, My) is needed for states that do not come from Context.map_stats")
    Mx, My = _two_ints(cells, what, "cells must be (Mx, My)")
    _stats_state(dst, Mx, My, what, "dst")
    _stats_state(src, Mx, My, what, "src")
    if dst.data_ptr() == src.data_ptr():
        raise ValueError(f"{what}: dst and src must be two states")
    return Mx, My


def _map_stats_finish_args(state, cells, mode, sense, k, rank, empty, ref):
    """the checks of Context.map_stats_finish that need no device: (Mx, My, the mode's value, the sense's value, k, rank, empty)"""
    what = "Context.map_stats_finish"
    Mx, My = _two_ints(cells, what, "cells must be (Mx, My)")
    _stats_state(state, Mx, My, what)
    if mode not in CALIB_MODE:
        raise ValueError(f"{what}: mode must be one of {sorted(CALIB_MODE)}")
    if sense not in REGIONS_SENSE:
        raise ValueError(f"{what}: sense must be one of {sorted(REGIONS_SENSE)}")
    try:
        k, empty = float(k), float(empty)
        if isinstance(rank, bool) or int(rank) != rank:
            raise ValueError
        rank = int(rank)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: k and empty must be numbers and rank an int") from None
    with np.errstate(over="ignore"):
        finite = bool(np.isfinite(np.float32(k)))                                # (as a float: what the library receives)
    if not finite or not 1 <= rank <= 4:
        raise ValueError(f"{what}: k must be finite and rank in 1..4")
    if ref is not None and (not isinstance(ref, torch.Tensor) or ref.dtype != torch.float32 or tuple(ref.shape) != (Mx, My) or not ref.is_contiguous()):
        raise ValueError(f"{what}: ref must be a contiguous float32 tensor of shape {(Mx, My)}")
    return Mx, My, CALIB_MODE[mode], REGIONS_SENSE[sense], k, rank, empty


def _map_peak_args(map, ref, sense, peak, cell):
    """the checks of Context.map_peak that need no device: (map as [B][Mx][My], the sense's value)"""
    what = "Context.map_peak"
    m = _maps3(map, what)
    B, Mx, My = m.shape
    if sense not in REGIONS_SENSE:
        raise ValueError(f"{what}: sense must be one of {sorted(REGIONS_SENSE)}")
    if ref is not None and (not isinstance(ref, torch.Tensor) or ref.dtype != torch.float32 or tuple(ref.shape) != (Mx, My) or not ref.is_contiguous()):
        raise ValueError(f"{what}: ref must be a contiguous float32 tensor of shape {(Mx, My)}")
    if peak is not None and (not isinstance(peak, torch.Tensor) or peak.dtype != torch.float32 or tuple(peak.shape) != (B,) or not peak.is_contiguous()):
        raise ValueError(f"{what}: peak must be a contiguous float32 tensor of shape {(B,)}")
    if cell is not None and (not isinstance(cell, torch.Tensor) or cell.dtype != torch.int32 or tuple(cell.shape) != (B,) or not cell.is_contiguous()):
        raise ValueError(f"{what}: cell must be a contiguous int32 tensor of shape {(B,)}")
    return m, REGIONS_SENSE[sense]


WARP_INTERP = {"nearest": 0, "linear": 1}                    # AEFFT_WARP_NEAREST, AEFFT_WARP_LINEAR
WARP_BORDER = {"constant": 0, "replicate": 1, "reflect": 2}  # AEFFT_BORDER_CONSTANT, AEFFT_BORDER_REPLICATE, AEFFT_BORDER_REFLECT
_I32_MIN, _I32_MAX = -2 ** 31, 2 ** 31 - 1


def affine_q(m):
    """The Q24 coefficients aefft_image_warp_affine takes (aefft_affine_make; host arithmetic, no device): `m` is a 2 x 3 matrix or B of them
    (B x 2 x 3), destination pixel -> source position, u = m00 x + m01 y + m02, v = m10 x + m11 y + m12.  Returns the int64 array (B, 6),
    a[k] = m[k] * 2^24 rounded to nearest, ties to even; ValueError for what the library refuses (a non-finite entry, a scale above 32, an
    offset above 32768 pixels)."""
    what = "affine_q"
    try:
        a = np.ascontiguousarray(np.asarray(m, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the matrix must be numbers, 2 x 3 or B x 2 x 3") from None
    if a.shape == (2, 3):
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (2, 3) or a.shape[0] < 1:
        raise ValueError(f"{what}: the matrix must be 2 x 3 or B x 2 x 3; got shape {np.shape(m)}")
    rows = a.reshape(-1, 6)
    out = np.empty(rows.shape, np.int64)
    for k, row in enumerate(rows):
        q = Affine()
        if lib().aefft_affine_make(row.ctypes.data_as(C.POINTER(C.c_double)), C.byref(q)) != OK:
            raise ValueError(f"{what}: every entry must be finite, the four linear entries at most 32 and the two offsets at most 32768 pixels in "
                             f"magnitude; got {row.tolist()}")
        out[k] = list(q.a)
    return out


def _table_size(size, what):
    Wd, Hd = _two_ints(size, what, "size must be (Wd, Hd)")
    if not (1 <= Wd <= 8192 and 1 <= Hd <= 8192):
        raise ValueError(f"{what}: size must be in 1..8192 per axis")
    return Wd, Hd


def _table_q11(u, v, dead=None):
    """t = rint(2048 * u) clipped to int32, as the int32 table [Hd][Wd][2], x first; `dead` entries get INT32_MIN, which is outside any image"""
    t = np.stack([np.clip(np.rint(2048.0 * u), _I32_MIN, _I32_MAX), np.clip(np.rint(2048.0 * v), _I32_MIN, _I32_MAX)], axis=-1)
    t[~np.isfinite(t)] = _I32_MIN
    if dead is not None:
        t[dead] = _I32_MIN
    return np.ascontiguousarray(t.astype(np.int32))


def affine_table(m, size):
    """The table Context.image_remap takes for ONE affine (host numpy): exactly the (tx, ty) aefft_image_warp_affine forms from affine_q(m), in
    integer arithmetic -- the two calls then give the same bytes.  size = (Wd, Hd).  Returns np.int32 [Hd][Wd][2], x first."""
    what = "affine_table"
    Wd, Hd = _table_size(size, what)
    q = affine_q(m)
    if q.shape[0] != 1:
        raise ValueError(f"{what}: one 2 x 3 matrix")
    a = q[0]
    y, x = np.meshgrid(np.arange(Hd, dtype=np.int64), np.arange(Wd, dtype=np.int64), indexing="ij")
    # (within affine_q's ranges |U| < 2^43: neither the wrap nor the clamp of the definition is active)
    t = np.stack([(a[0] * x + a[1] * y + a[2] + 4096) >> 13, (a[3] * x + a[4] * y + a[5] + 4096) >> 13], axis=-1)
    return np.ascontiguousarray(np.clip(t, _I32_MIN, _I32_MAX).astype(np.int32))


def homography_table(Hm, size):
    """The table of a plane-to-plane homography (host numpy, float64): `Hm` is 3 x 3, destination pixel -> source position,
    u = (h00 x + h01 y + h02) / (h20 x + h21 y + h22) and v alike.  A non-positive denominator gives INT32_MIN for both entries, which is outside
    any image.  size = (Wd, Hd).  Returns np.int32 [Hd][Wd][2], t = rint(2048 u) clipped to int32."""
    what = "homography_table"
    Wd, Hd = _table_size(size, what)
    h = np.asarray(Hm, dtype=np.float64)
    if h.shape != (3, 3) or not np.isfinite(h).all():
        raise ValueError(f"{what}: Hm must be a finite 3 x 3 matrix")
    y, x = np.meshgrid(np.arange(Hd, dtype=np.float64), np.arange(Wd, dtype=np.float64), indexing="ij")
    den = h[2, 0] * x + h[2, 1] * y + h[2, 2]
    dead = ~(den > 0.0)
    den = np.where(dead, 1.0, den)
    return _table_q11((h[0, 0] * x + h[0, 1] * y + h[0, 2]) / den, (h[1, 0] * x + h[1, 1] * y + h[1, 2]) / den, dead)


def undistort_table(K, dist, size, new_K=None):
    """The table that undoes a lens (host numpy, float64): the Brown-Conrady forward model evaluated at each ideal destination pixel --
    cv::initUndistortRectifyMap without the rotation; there is no inversion, the undistort map IS the forward model.  `K` is the 3 x 3 camera
    matrix (fx, fy, cx, cy are read from it), dist = (k1, k2, p1, p2[, k3]), new_K the camera matrix of the ideal image (default K),
    size = (Wd, Hd).  With xn = (x - cx') / fx', yn = (y - cy') / fy', r2 = xn^2 + yn^2 and c = 1 + k1 r2 + k2 r2^2 + k3 r2^3:
    xd = xn c + 2 p1 xn yn + p2 (r2 + 2 xn^2), yd = yn c + p1 (r2 + 2 yn^2) + 2 p2 xn yn, u = fx xd + cx, v = fy yd + cy.
    Returns np.int32 [Hd][Wd][2]."""
    what = "undistort_table"
    Wd, Hd = _table_size(size, what)
    k = np.asarray(K, dtype=np.float64)
    n = k if new_K is None else np.asarray(new_K, dtype=np.float64)
    d = np.asarray(dist, dtype=np.float64).reshape(-1)
    if k.shape != (3, 3) or n.shape != (3, 3) or d.size not in (4, 5) or not (np.isfinite(k).all() and np.isfinite(n).all() and np.isfinite(d).all()):
        raise ValueError(f"{what}: K and new_K must be finite 3 x 3 matrices and dist (k1, k2, p1, p2[, k3])")
    if k[0, 0] == 0 or k[1, 1] == 0 or n[0, 0] == 0 or n[1, 1] == 0:
        raise ValueError(f"{what}: the focal lengths must not be zero")
    k1, k2, p1, p2 = d[:4]
    k3 = d[4] if d.size == 5 else 0.0
    y, x = np.meshgrid(np.arange(Hd, dtype=np.float64), np.arange(Wd, dtype=np.float64), indexing="ij")
    xn, yn = (x - n[0, 2]) / n[0, 0], (y - n[1, 2]) / n[1, 1]
    r2 = xn * xn + yn * yn
    c = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = xn * c + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
    yd = yn * c + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
    return _table_q11(k[0, 0] * xd + k[0, 2], k[1, 1] * yd + k[1, 2])


def _warp_common(what, image, interp, border, value, out, Wd, Hd):
    """what image_warp and image_remap share: (the image as [B][H][W][D], pitch, stride, interp value, border value, border_value)"""
    img, pitch, stride = _resize_layout(image, what)
    B, H, W, D = img.shape
    if not 1 <= D <= 4 or W > 8192 or H > 8192:
        raise ValueError(f"{what}: D must be 1..4 and W, H in 1..8192")
    if interp not in WARP_INTERP:
        raise ValueError(f"{what}: interp must be one of {sorted(WARP_INTERP)}")
    if border not in WARP_BORDER:
        raise ValueError(f"{what}: border must be one of {sorted(WARP_BORDER)}")
    try:
        vals = [value] * D if isinstance(value, (int, np.integer)) and not isinstance(value, bool) else list(value)
        if len(vals) != D or any(isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 255 for v in vals):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{what}: value must be an int in 0..255 or one per channel ({D})") from None
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 4 or tuple(out.shape) != (B, Hd, Wd, D)):
        raise ValueError(f"{what}: out must be a uint8 tensor of shape {(B, Hd, Wd, D)}")
    return img, pitch, stride, WARP_INTERP[interp], WARP_BORDER[border], sum(int(v) << (8 * d) for d, v in enumerate(vals))


def _image_warp_args(image, matrix, size, interp, border, value, out):
    """the checks of Context.image_warp that need no device: (the image as [B][H][W][D], pitch, stride, the affines -- an int64 numpy array
    (nm, 6) to upload, or the caller's int64 tensor as it is --, (Wd, Hd), interp value, border value, border_value)"""
    what = "Context.image_warp"
    if image.dtype != torch.uint8 or image.dim() not in (3, 4):
        raise ValueError(f"{what}: the image must be a uint8 tensor [B][H][W][D] or [H][W][D]")
    B = image.shape[0] if image.dim() == 4 else 1
    H, W = image.shape[-3], image.shape[-2]
    Wd, Hd = (W, H) if size is None else _table_size(size, what)
    if isinstance(matrix, torch.Tensor) and matrix.dtype == torch.int64:
        q = matrix
        if q.dim() != 2 or q.shape[1] != 6 or not q.is_contiguous():
            raise ValueError(f"{what}: an int64 matrix tensor must be contiguous, (nm, 6)")
    else:
        q = affine_q(matrix.detach().cpu().numpy() if isinstance(matrix, torch.Tensor) else matrix)
    if q.shape[0] not in (1, B):
        raise ValueError(f"{what}: {q.shape[0]} matrices for {B} images (one for the batch, or one per image)")
    img, pitch, stride, i, b, v = _warp_common(what, image, interp, border, value, out, Wd, Hd)
    return img, pitch, stride, q, (Wd, Hd), i, b, v


def _image_remap_args(image, table, interp, border, value, out):
    """the checks of Context.image_remap that need no device: (the image as [B][H][W][D], pitch, stride, (Wd, Hd), interp value, border value,
    border_value)"""
    what = "Context.image_remap"
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 3 or table.shape[2] != 2 or not table.is_contiguous() or min(table.shape) < 1:
        raise ValueError(f"{what}: table must be a contiguous int32 tensor [Hd][Wd][2]")
    Hd, Wd = int(table.shape[0]), int(table.shape[1])
    if Wd > 8192 or Hd > 8192:
        raise ValueError(f"{what}: the table's size must be in 1..8192 per axis")
    img, pitch, stride, i, b, v = _warp_common(what, image, interp, border, value, out, Wd, Hd)
    return img, pitch, stride, (Wd, Hd), i, b, v


REGISTER_WINDOW = {"hann": 0, "nowindow": 1}                  # AEFFT_REGISTER_HANN, AEFFT_REGISTER_NOWINDOW
# aefft_shift as a numpy record
SHIFT = np.dtype([("dx", "<f4"), ("dy", "<f4"), ("response", "<f4"), ("cell", "<i4")])


class RegisterRef:
    """What Context.frames_register_ref returns: the reference spectra [nref][Nx][Ny/2+1] (complex64, on the device), the window they were made
    with and the sizes"""

    def __init__(self, spec, window, D, Nx, Ny):
        self.spec, self.window, self.D, self.Nx, self.Ny = spec, window, D, Nx, Ny
        self.nref = spec.shape[0]


def _register_args(frames, ref, cutoff, min_response, scale):
    """the checks of Context.frames_register that need no device: (B, D, Nx, Ny, scale_x, scale_y)"""
    what = "Context.frames_register"
    B, D, Nx, Ny = _frames4(frames, what)
    if not isinstance(ref, RegisterRef):
        raise ValueError(f"{what}: ref must be what Context.frames_register_ref returned")
    if (ref.D, ref.Nx, ref.Ny) != (D, Nx, Ny) or ref.nref not in (1, B):
        raise ValueError(f"{what}: the reference was made from {ref.nref} frames of D, Nx, Ny = {(ref.D, ref.Nx, ref.Ny)}; the frames need 1 or {B} of {(D, Nx, Ny)}")
    if not 0.0 < float(cutoff) <= 1.0:
        raise ValueError(f"{what}: cutoff must be in (0, 1]")
    if math.isnan(float(min_response)):
        raise ValueError(f"{what}: min_response must not be NaN")
    try:
        sx, sy = (float(v) for v in scale)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: scale must be (scale_x, scale_y)") from None
    if not (0.0 < sx <= 32.0 and 0.0 < sy <= 32.0):
        raise ValueError(f"{what}: scale_x and scale_y must be in (0, 32]")
    return B, D, Nx, Ny, sx, sy


class Context:
    """aefft_ctx on torch's current device, enqueuing on torch's current stream by default."""

    def __init__(self, device=None, use_torch_stream=True):
        import torch
        if not torch.cuda.is_available():
            raise AefftError("no MI355X visible (torch.cuda.is_available() is False); aefft has no CPU path")
        self.torch = torch
        self.device = torch.cuda.current_device() if device is None else int(device)
        torch.cuda.set_device(self.device)
        self.L = lib()
        h = C.c_void_p()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if use_torch_stream else None
        rc = self.L.aefft_ctx_create(C.byref(h), self.device, stream, 0 if use_torch_stream else 1)
        if rc != OK:
            raise AefftError(f"aefft_ctx_create failed with code {rc}")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.aefft_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        if _exiting:      # interpreter shutdown: the HIP runtime may already be gone; the process frees everything
            return
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != OK:
            raise AefftError(f"aefft error {rc}: {self.L.aefft_last_error(self.h).decode()}")

    def sync(self):
        self.check(self.L.aefft_sync(self.h))

    def partition(self, side_cus):
        """aefft_ctx_partition: CU-masked streams -- the side streams get `side_cus` compute units, the context stream the rest"""
        self.check(self.L.aefft_ctx_partition(self.h, int(side_cus)))

    def torch_stream(self):
        """The library's stream as a torch stream object (so collectives / torch ops can be ordered on it)."""
        ptr = self.L.aefft_stream(self.h)
        if not ptr:
            return self.torch.cuda.default_stream(self.device)
        return self.torch.cuda.ExternalStream(ptr, device=f"cuda:{self.device}")

    # ---- helpers on torch tensors (float32 / complex64, contiguous, on this device) ----
    def empty(self, *shape, dtype=None):
        t = self.torch
        return t.empty(*shape, dtype=dtype or t.float32, device=f"cuda:{self.device}")

    def dev(self, a, dtype=None):
        t = self.torch
        a = np.ascontiguousarray(a)
        if np.iscomplexobj(a):
            a = a.astype(np.complex64)
        else:
            a = a.astype(np.float32)
        return t.from_numpy(a).to(f"cuda:{self.device}")

    # ---- op level ----
    def r2c(self, x):
        *lead, Nx, Ny = x.shape
        planes = int(np.prod(lead)) if lead else 1
        X = self.empty(*lead, Nx, Ny // 2 + 1, dtype=self.torch.complex64)
        self.check(self.L.aefft_r2c(self.h, _ptr(x), _ptr(X), planes, Nx, Ny))
        return X

    def c2r(self, X, Ny, scale=None):
        *lead, Nx, Nyr = X.shape
        planes = int(np.prod(lead)) if lead else 1
        x = self.empty(*lead, Nx, Ny)
        s = 1.0 / (Nx * Ny) if scale is None else scale
        self.check(self.L.aefft_c2r(self.h, _ptr(X), _ptr(x), planes, Nx, Ny, s))
        return x

    def pool(self, X, Ny, scale):
        *lead, Nx, Nyr = X.shape
        planes = int(np.prod(lead)) if lead else 1
        a = abs(scale)
        nx, ny = (Nx // a, Ny // a) if scale > 0 else (Nx * a, Ny * a)
        Xs = self.empty(*lead, nx, ny // 2 + 1, dtype=self.torch.complex64)
        onx, ony = C.c_int(), C.c_int()
        self.check(self.L.aefft_pool(self.h, _ptr(X), _ptr(Xs), planes, Nx, Ny, scale, C.byref(onx), C.byref(ony)))
        assert (onx.value, ony.value) == (nx, ny)
        return Xs, nx, ny

    def r2c_pool(self, x, scale):
        *lead, Nx, Ny = x.shape
        planes = int(np.prod(lead)) if lead else 1
        Xs = self.empty(*lead, Nx // scale, Ny // scale // 2 + 1, dtype=self.torch.complex64)
        self.check(self.L.aefft_r2c_pool(self.h, _ptr(x), _ptr(Xs), planes, Nx, Ny, scale))
        return Xs

    def unpool_c2r(self, Xs, Nys, scale, out_scale):
        *lead, Nxs, _ = Xs.shape
        planes = int(np.prod(lead)) if lead else 1
        a = -scale
        x = self.empty(*lead, Nxs * a, Nys * a)
        self.check(self.L.aefft_unpool_c2r(self.h, _ptr(Xs), _ptr(x), planes, Nxs, Nys, scale, out_scale))
        return x

    def kernel_spectrum(self, k, Nx, Ny):
        nA, nB, Nk, Nl = k.shape
        K = self.empty(nA, nB, Nx, Ny // 2 + 1, dtype=self.torch.complex64)
        self.check(self.L.aefft_kernel_spectrum(self.h, _ptr(k), _ptr(K), nA, nB, Nk, Nl, Nx, Ny))
        return K

    def kernel_export(self, K, Nk, Nl, Ny):
        nA, nB, Nx, _ = K.shape
        k = self.empty(nA, nB, Nk, Nl)
        self.check(self.L.aefft_kernel_export(self.h, _ptr(K), _ptr(k), nA, nB, Nk, Nl, Nx, Ny))
        return k

    def conv(self, X, Cs, bias, Ny):
        B, dD, Nx, _ = X.shape
        dM = Cs.shape[0]
        O = self.empty(B, dM, Nx, Ny // 2 + 1, dtype=self.torch.complex64)
        self.check(self.L.aefft_conv(self.h, _ptr(X), _ptr(Cs), _ptr(bias), _ptr(O), B, dM, dD, Nx, Ny))
        return O

    def gradient(self, Xin, Xout, O, Cs, Fs, b, Ny):
        B, dD, Nx, Nyr = Xin.shape
        dM = Cs.shape[0]
        c64 = self.torch.complex64
        dc = self.empty(dM, dD, Nx, Nyr, dtype=c64); df = self.empty(dD, dM, Nx, Nyr, dtype=c64)
        db = self.empty(dM); dp = self.empty(dD)
        self.check(self.L.aefft_gradient(self.h, _ptr(Xin), _ptr(Xout), _ptr(O), _ptr(Cs), _ptr(Fs), _ptr(b),
                                         _ptr(dc), _ptr(df), _ptr(db), _ptr(dp), B, dM, dD, Nx, Ny))
        return dc, df, db, dp

    def mse(self, T, O, dM, Ny):
        B, dD, Nx, _ = T.shape
        out = self.empty(1)
        self.check(self.L.aefft_mse(self.h, _ptr(T), _ptr(O), _ptr(out), B, dM, dD, Nx, Ny))
        return out

    def update(self, c, f, b, p, Cs, Fs, dc, df, db, dp, Dc, Df, Db, Dp, Ny, dele, maxdiff):
        dM, dD, Nk, Nl = c.shape
        Nx = Cs.shape[2]
        self.check(self.L.aefft_update(self.h, _ptr(c), _ptr(f), _ptr(b), _ptr(p), _ptr(Cs), _ptr(Fs), _ptr(dc), _ptr(df),
                                       _ptr(db), _ptr(dp), _ptr(Dc), _ptr(Df), _ptr(Db), _ptr(Dp),
                                       dM, dD, Nx, Ny, Nk, Nl, dele, maxdiff))

    def magnitude(self, X, Ny, ch, shift=False):
        *lead, Nx, Nyr = X.shape
        planes = int(np.prod(lead)) if lead else 1
        mag = self.empty(*lead, Nx, Ny)
        self.check(self.L.aefft_magnitude(self.h, _ptr(X), _ptr(mag), planes, ch, Nx, Ny, 1 if shift else 0))
        return mag

    def conv_spatial(self, x, c, b, semantics="gpu"):
        B, dD, Nx, Ny = x.shape
        dM, _, Nk, Nl = c.shape
        out = self.empty(B, dM, Nx, Ny)
        self.check(self.L.aefft_conv_spatial(self.h, _ptr(x), _ptr(out), _ptr(c), _ptr(b), B, dD, dM, Nx, Ny, Nk, Nl,
                                             0 if semantics == "gpu" else 1))
        return out

    def pool_spatial(self, x, out_shape, scale):
        """netlib.cpp Pool on the device: x [..., Nxi, Nyi] -> zeros(out_shape) filled where the reference writes."""
        import torch
        out = torch.zeros(tuple(x.shape[:-2]) + tuple(out_shape), dtype=torch.float32, device=x.device)
        planes = int(np.prod(x.shape[:-2]))
        self.check(self.L.aefft_pool_spatial(self.h, _ptr(x), _ptr(out), planes, x.shape[-2], x.shape[-1], out_shape[0], out_shape[1], scale))
        return out

    def pool_conv_spatial(self, x, c, b, scale, semantics="gpu", want_pooled=True):
        """Pool(scale) + Conv_gpu in one launch; returns (pooled layer or None, conv output)."""
        B, dD, Nxi, Nyi = x.shape
        dM, _, Nk, Nl = c.shape
        Nx, Ny = Nxi // scale, Nyi // scale
        pooled = self.empty(B, dD, Nx, Ny) if want_pooled else None
        out = self.empty(B, dM, Nx, Ny)
        self.check(self.L.aefft_pool_conv_spatial(self.h, _ptr(x), _ptr(pooled), _ptr(out), _ptr(c), _ptr(b), B, dD, dM, Nx, Ny, scale, Nk, Nl,
                                                  0 if semantics == "gpu" else 1))
        return pooled, out

    def backprop_spatial(self, x, out, hin, c, b, f, p, mom, grads, delmax, alpha, tied=False, semantics="gpu"):
        """mom = (dc, db, df, dp), grads = (ddc, ddb, ddf, ddp): torch tensors updated in place."""
        B, dD, Nx, Ny = x.shape
        dM, _, Nk, Nl = c.shape
        dc, db, df, dp = mom
        ddc, ddb, ddf, ddp = grads
        self.check(self.L.aefft_backprop_spatial(self.h, _ptr(x), _ptr(out), _ptr(hin), _ptr(c), _ptr(b), _ptr(f), _ptr(p),
                                                 _ptr(dc), _ptr(db), _ptr(df), _ptr(dp), _ptr(ddc), _ptr(ddb), _ptr(ddf), _ptr(ddp),
                                                 B, dD, dM, Nx, Ny, Nk, Nl, delmax, alpha, 1 if tied else 0,
                                                 {"gpu": 0, "cpu": 1, "cuda_compat": 2}[semantics]))

    def step_spatial(self, x, c, b, f, p, mom, grads, delmax, alpha, tied=False, semantics="gpu", hin=None, out=None):
        """Conv_gpu + Conv_gpu + backprop_gpu[_cc] in one call (aefft_step_spatial); returns (hin, out)."""
        B, dD, Nx, Ny = x.shape
        dM, _, Nk, Nl = c.shape
        hin = self.empty(B, dM, Nx, Ny) if hin is None else hin
        out = self.empty(B, dD, Nx, Ny) if out is None else out
        dc, db, df, dp = mom
        ddc, ddb, ddf, ddp = grads
        self.check(self.L.aefft_step_spatial(self.h, _ptr(x), _ptr(hin), _ptr(out), _ptr(c), _ptr(b), _ptr(f), _ptr(p),
                                             _ptr(dc), _ptr(db), _ptr(df), _ptr(dp), _ptr(ddc), _ptr(ddb), _ptr(ddf), _ptr(ddp),
                                             B, dD, dM, Nx, Ny, Nk, Nl, delmax, alpha, 1 if tied else 0, {"gpu": 0, "cpu": 1}[semantics]))
        return hin, out

    # ---- image boundary ----
    def image_to_frames(self, image, out=None, dtype=torch.uint8):
        """ImageToSpin_C on the device (aefft_image_to_frames): `image` is a uint8 device tensor [B][Ny][Nx][D] of interleaved image rows (or
        [Ny][Nx][D] for one image), contiguous or a row-padded view (stride(-3) = pitch >= Nx * D; ValueError otherwise).  Returns, or fills
        `out` with, the planar frames [B][D][Nx][Ny] of `dtype` uint8 or float32: frames[b][d][i][j] = image[b][j][i][d].  One launch, nothing
        waits for the device."""
        img, pitch = _image_layout(image, "Context.image_to_frames")
        B, Ny, Nx, D = img.shape
        if out is None:
            if dtype not in (torch.uint8, torch.float32):
                raise ValueError("Context.image_to_frames: dtype must be torch.uint8 or torch.float32")
            out = self.empty(B, D, Nx, Ny, dtype=dtype)
        elif out.dtype not in (torch.uint8, torch.float32) or tuple(out.shape) != (B, D, Nx, Ny) or not out.is_contiguous():
            raise ValueError(f"Context.image_to_frames: out must be a contiguous uint8 or float32 tensor of shape {(B, D, Nx, Ny)}")
        self.check(self.L.aefft_image_to_frames(self.h, _ptr(img), pitch, _ptr(out), int(_is_u8(out)), B, D, Nx, Ny))
        return out

    def frames_to_image(self, frames, out=None):
        """SpinToImage_C on the device (aefft_frames_to_image): `frames` is uint8 or float32 [B][D][Nx][Ny]; float values become
        clamp(round(v), 0, 255) as Net.infer's uint8 reconstruction does.  Returns, or fills `out` with, the uint8 image rows [B][Ny][Nx][D];
        `out` may be a row-padded view as for image_to_frames (its pad bytes are not written).  One launch, nothing waits for the device."""
        if frames.dtype not in (torch.uint8, torch.float32) or frames.dim() != 4 or not frames.is_contiguous():
            raise ValueError("Context.frames_to_image: frames must be a contiguous uint8 or float32 tensor [B][D][Nx][Ny]")
        B, D, Nx, Ny = frames.shape
        if out is None:
            out = self.empty(B, Ny, Nx, D, dtype=torch.uint8)
        img, pitch = _image_layout(out, "Context.frames_to_image")
        if tuple(img.shape) != (B, Ny, Nx, D):
            raise ValueError(f"Context.frames_to_image: out must have shape {(B, Ny, Nx, D)}")
        self.check(self.L.aefft_frames_to_image(self.h, _ptr(frames), int(_is_u8(frames)), _ptr(img), pitch, B, D, Nx, Ny))
        return out

    def image_resize_to_frames(self, image, size, mode="linear", out=None, dtype=torch.uint8):
        """resize + ImageToSpin_C on the device (aefft_image_resize_to_frames): `image` is a uint8 device tensor [B][H][W][D] of interleaved image
        rows (or [H][W][D]) of ANY size -- contiguous, row-padded, or a region of interest big[:, y0:y1, x0:x1] of a larger batch (stride(-1) == 1,
        stride(-2) == D, stride(-3) >= W * D, any sufficient batch stride; ValueError otherwise).  size = (Nx, Ny), the frames' columns and rows.
        mode "linear" (cv::resize's default geometry, any size to any size) or "area" (the exact box average; Nx <= W, Ny <= H).  Returns, or
        fills `out` with, the planar frames [B][D][Nx][Ny] of `dtype` uint8 or float32.  All-integer arithmetic (include/aefft.h).  One launch,
        nothing waits for the device."""
        what = "Context.image_resize_to_frames"
        img, pitch, stride = _resize_layout(image, what)
        B, H, W, D = img.shape
        if mode not in RESIZE_MODES:
            raise ValueError(f"{what}: mode must be one of {sorted(RESIZE_MODES)}")
        Nx, Ny = _two_ints(size, what, "size must be (Nx, Ny)")
        if out is None:
            if dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"{what}: dtype must be torch.uint8 or torch.float32")
            if Nx < 1 or Ny < 1:
                raise ValueError(f"{what}: size must be positive")
            out = self.empty(B, D, Nx, Ny, dtype=dtype)
        elif out.dtype not in (torch.uint8, torch.float32) or tuple(out.shape) != (B, D, Nx, Ny) or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous uint8 or float32 tensor of shape {(B, D, Nx, Ny)}")
        self.check(self.L.aefft_image_resize_to_frames(self.h, _ptr(img), pitch, stride, W, H, RESIZE_MODES[mode], _ptr(out), int(_is_u8(out)), B, D, Nx, Ny))
        return out

    def frames_resize_to_image(self, frames, size, mode="linear", out=None):
        """SpinToImage_C + resize on the device (aefft_frames_resize_to_image), the mirror of image_resize_to_frames: `frames` is uint8 or float32
        [B][D][Nx][Ny] (float values become pixels first, as in frames_to_image); size = (W, H), the image's columns and rows; mode "linear" (any
        size to any size) or "area" (the exact box average; W <= Nx, H <= Ny).  Returns, or fills `out` with, the uint8 image rows [B][H][W][D];
        `out` may be a row-padded view or a region of interest big[:, y0:y1, x0:x1] of a larger batch (bytes outside it are not written;
        ValueError for layouts the C call cannot describe).  All-integer arithmetic (include/aefft.h).  One launch, nothing waits for the device."""
        W, H, m = _frames_resize_args(frames, size, mode, out)
        B, D, Nx, Ny = frames.shape
        if out is None:
            out = self.empty(B, H, W, D, dtype=torch.uint8)
        img, pitch, stride = _resize_layout(out, "Context.frames_resize_to_image")
        self.check(self.L.aefft_frames_resize_to_image(self.h, _ptr(frames), int(_is_u8(frames)), Nx, Ny, m, _ptr(img), pitch, stride, W, H, B, D))
        return out

    def map_overlay(self, map, image, lut, lo, hi, alpha=128, smooth=True):
        """A heat map onto images, IN PLACE (aefft_map_overlay_image): `map` is float32 [B][Mx][My] or [Mx][My] as Net.score_map / Net.ssim_map
        return it; `image` uint8 [B][H][W][D] or [H][W][D], contiguous, row-padded or a region of interest; `lut` a uint8 device tensor [256][D]
        (heat_lut gives a default).  k = clamp(round((m - lo) * 255 / (hi - lo)), 0, 255) per map entry (hi < lo inverts the scale), carried to
        the pixels bilinearly (smooth) or per tile, then image = (alpha * lut[k] + (256 - alpha) * image + 128) >> 8 with alpha in 0..256.
        Returns `image`.  One launch, nothing waits for the device."""
        m, img, pitch, stride = _overlay_args(map, image, lut, lo, hi, alpha)
        B, H, W, D = img.shape
        self.check(self.L.aefft_map_overlay_image(self.h, _ptr(m), m.shape[1], m.shape[2], float(lo), float(hi), 1 if smooth else 0, _ptr(lut), int(alpha),
                                                  _ptr(img), pitch, stride, W, H, B, D))
        return image

    def image_compare_map(self, a, b, cells, metric="mse", map=None, score=None):
        """Where two images differ, at their own resolution (aefft_image_compare_map): `a` and `b` are uint8 device tensors [B][H][W][D] or
        [H][W][D] of one shape, each contiguous, row-padded or a region of interest with its own pitch and stride (b may be a itself);
        cells = (Mx, My), the grid of at most 64 x 64-pixel cells (cells_for_tile gives it from a cell size).  map[b][I][J] is the mean squared
        error ("mse") or the mean SSIM of the channels ("ssim", data range 255) over the pixels x, y with floor(x Mx / W) = I and
        floor(y My / H) = J -- what map_overlay(smooth=False) colours with that entry --, score[b] the pixel-weighted mean of the map; both are
        defined bit for bit from integer sums (include/aefft.h).  `map` (float32 [B][Mx][My]) and `score` (float32 [B]) are allocated when None;
        score=False skips the score and its launch.  Nothing waits for the device.  Returns (map, score)."""
        ia, pa, sa, ib, pb, sb, (Mx, My), m = _image_compare_args(a, b, cells, metric, map, score)
        B, H, W, D = ia.shape
        if map is None:
            map = self.empty(B, Mx, My)
        if score is None:
            score = self.empty(B)
        elif score is False:
            score = None
        self.check(self.L.aefft_image_compare_map(self.h, _ptr(ia), pa, sa, _ptr(ib), pb, sb, W, H, B, D, m, Mx, My, _ptr(map), _ptr(score)))
        return map, score

    def map_regions(self, map, lo, hi=None, ref=None, sense="above", connectivity=8, min_area=1, max_regions=256, labels=None, regions=None, count=None):
        """Detections from a map (aefft_map_regions): `map` is float32 [B][Mx][My] or [Mx][My] as Net.score_map, Net.ssim_map and
        Context.image_compare_map return it, `ref` an optional per-cell baseline [Mx][My] subtracted first.  A cell is foreground when
        v >= lo (sense "above") or v <= lo ("below": an SSIM map), strong when it passes `hi` too (hi=None: hi = lo, a plain threshold); the
        4- or 8-connected components with a strong cell and at least `min_area` cells are numbered 1..n in the order of their first cell
        (index I * My + J).  labels (int32 [B][Mx][My]) holds the numbers, 0 elsewhere; regions (int32 [B][max_regions][8], the bytes of
        aefft_region: regions.cpu().numpy().view(REGION)[..., 0]) the first min(n, max_regions) boxes with area and peak, the rest untouched
        (zeros when allocated here); count (int32 [B]) holds n.  max_regions=0 skips the regions (None is returned for them).  Everything is
        allocated when None; the workspace is cached per shape.  Six launches, nothing waits for the device.  Returns (labels, regions, count)."""
        m, lo, hi, s, conn, min_area, max_regions = _map_regions_args(map, lo, hi, ref, sense, connectivity, min_area, max_regions, labels, regions, count)
        B, Mx, My = m.shape
        if labels is None:
            labels = self.empty(B, Mx, My, dtype=torch.int32)
        if regions is None and max_regions:
            regions = torch.zeros(B, max_regions, 8, dtype=torch.int32, device=m.device)
        if count is None:
            count = self.empty(B, dtype=torch.int32)
        cache = self.__dict__.setdefault("_regions_work", {})
        work = cache.get((B, Mx, My))
        if work is None:
            work = cache[(B, Mx, My)] = self.empty(self.L.aefft_map_regions_workspace(Mx, My, B), dtype=torch.uint8)
        self.check(self.L.aefft_map_regions(self.h, _ptr(m), _ptr(ref), Mx, My, B, s, lo, hi, conn, min_area, _ptr(labels), _ptr(regions), max_regions,
                                            _ptr(count), _ptr(work), work.numel()))
        return labels, regions, count

    def map_stats(self, Mx, My):
        """An empty calibration state for maps of Mx x My cells: a zeroed uint8 device tensor of aefft_map_stats_bytes(Mx, My) bytes (all-zero
        bytes are the empty state; map_stats_view shows its planes).  The grid is noted on the tensor as `cells` for map_stats_merge."""
        Mx, My = _two_ints((Mx, My), "Context.map_stats", "Mx, My must be ints")
        need = self.L.aefft_map_stats_bytes(Mx, My)
        if not need:
            raise ValueError("Context.map_stats: Mx, My must be in 1..1024")
        state = torch.zeros(need, dtype=torch.uint8, device=f"cuda:{self.device}")
        state.cells = (Mx, My)
        return state

    def map_stats_update(self, state, map):
        """The maps of nominal footage enter a calibration state (aefft_map_stats_update): `map` is float32 [B][Mx][My] or [Mx][My] as the map
        calls return it, `state` what map_stats(Mx, My) gave.  Per cell, in ascending b: a non-finite value is skipped; otherwise the sums of the
        values and of their squares (double), the count and the four largest and four smallest values take it in.  In place, one launch,
        nothing waits for the device.  Returns `state`."""
        m = _map_stats_update_args(state, map)
        B, Mx, My = m.shape
        self.check(self.L.aefft_map_stats_update(self.h, _ptr(m), Mx, My, B, _ptr(state), state.numel()))
        return state

    def map_stats_merge(self, dst, src, cells=None):
        """Two sessions' or two ranks' states as one (aefft_map_stats_merge): `src` enters `dst` -- the sums and counts add, the extremes are the
        four largest and smallest of both.  cells=(Mx, My) is needed only for states that do not come from map_stats.  Returns `dst`."""
        Mx, My = _map_stats_merge_args(dst, src, cells)
        self.check(self.L.aefft_map_stats_merge(self.h, _ptr(dst), _ptr(src), Mx, My, min(dst.numel(), src.numel())))
        return dst

    def map_stats_finish(self, state, cells, mode="rank", sense="above", k=3.0, rank=1, empty=float("inf"), ref=None):
        """The baseline map_regions takes as `ref`, out of a calibration state (aefft_map_stats_finish): cells = (Mx, My).  mode "rank": the
        rank-th largest (sense "above") or smallest ("below") value each cell saw, rank in 1..4 -- the nominal footage's maximum with rank - 1
        outliers tolerated, exact; mode "sigma": mean + k * standard deviation in double (k negative for "below").  A cell that counted nothing
        gets `empty` (inf: never foreground under "above").  `ref` (float32 [Mx][My]) is allocated when None.  Returns `ref`."""
        Mx, My, m, s, k, rank, empty = _map_stats_finish_args(state, cells, mode, sense, k, rank, empty, ref)
        if ref is None:
            ref = self.empty(Mx, My)
        self.check(self.L.aefft_map_stats_finish(self.h, _ptr(state), state.numel(), Mx, My, m, s, k, rank, empty, _ptr(ref)))
        return ref

    def map_peak(self, map, ref=None, sense="above", peak=None, cell=None):
        """The per-image peak of map - ref (aefft_map_peak): the image-level anomaly score, and over nominal footage the number map_regions' `hi`
        is chosen from.  `map` is float32 [B][Mx][My] or [Mx][My], `ref` an optional baseline [Mx][My]; peak[b] (float32 [B]) is the largest
        (sense "above") or smallest ("below") value over the cells that are not NaN, cell[b] (int32 [B]) the smallest index I * My + J that
        attains it; an image of NaN only gives NaN and -1.  One launch, nothing waits for the device.  Returns (peak, cell)."""
        m, s = _map_peak_args(map, ref, sense, peak, cell)
        B, Mx, My = m.shape
        if peak is None:
            peak = self.empty(B)
        if cell is None:
            cell = self.empty(B, dtype=torch.int32)
        self.check(self.L.aefft_map_peak(self.h, _ptr(m), _ptr(ref), Mx, My, B, s, _ptr(peak), _ptr(cell)))
        return peak, cell

    def image_warp(self, image, matrix, size=None, interp="linear", border="constant", value=0, out=None):
        """Images through an affine transform (aefft_image_warp_affine), one launch: `image` is a uint8 device tensor [B][H][W][D] or [H][W][D],
        contiguous, row-padded or a region of interest; `matrix` maps a DESTINATION pixel to the source position it samples (cv::warpAffine
        with WARP_INVERSE_MAP) -- a 2 x 3 matrix for the batch or B x 2 x 3, one per image, as floats (quantised by affine_q and uploaded), or
        an int64 device tensor (nm, 6) of Q24 coefficients used as it is (nothing is copied: the pose stays on the device).  size = (Wd, Hd)
        defaults to the source's size; interp "nearest" or "linear"; border "constant" (`value`: an int for all channels or one per
        channel), "replicate" or "reflect".  Defined bit for bit in integer arithmetic (include/aefft.h).  `out` (uint8 [B][Hd][Wd][D], any
        pitch) is allocated when None.  Returns out."""
        img, pitch, stride, q, (Wd, Hd), i, b, v = _image_warp_args(image, matrix, size, interp, border, value, out)
        B, H, W, D = img.shape
        if not isinstance(q, torch.Tensor):
            q = torch.from_numpy(q).to(img.device)
        if out is None:
            out = self.empty(B, Hd, Wd, D, dtype=torch.uint8)
        o, opitch, ostride = _resize_layout(out, "Context.image_warp: out")
        self.check(self.L.aefft_image_warp_affine(self.h, _ptr(img), pitch, stride, W, H, _ptr(q), q.shape[0], i, b, v, _ptr(o), opitch, ostride, Wd, Hd, B, D))
        return out

    def image_remap(self, image, table, interp="linear", border="constant", value=0, out=None):
        """Images through a per-pixel table (aefft_image_remap: a lens, a homography), one launch: `table` is an int32 device tensor
        [Hd][Wd][2] of source positions times 2048, x first, shared by the batch (undistort_table, homography_table and affine_table make
        it on the host; any int32 value is legal).  `image`, interp, border, value and out as in image_warp.  Returns out."""
        img, pitch, stride, (Wd, Hd), i, b, v = _image_remap_args(image, table, interp, border, value, out)
        B, H, W, D = img.shape
        if out is None:
            out = self.empty(B, Hd, Wd, D, dtype=torch.uint8)
        o, opitch, ostride = _resize_layout(out, "Context.image_remap: out")
        self.check(self.L.aefft_image_remap(self.h, _ptr(img), pitch, stride, W, H, _ptr(table), i, b, v, _ptr(o), opitch, ostride, Wd, Hd, B, D))
        return out

    def _register_work(self, Nx, Ny, B, what):
        need = self.L.aefft_register_workspace(Nx, Ny, B)
        if not need:
            raise ValueError(f"{what}: Nx, Ny must be powers of two in 8..2048 or even sizes in 10..2048 with no prime factor above 5, and B * Nx * Ny below 2^29")
        return self.empty(need, dtype=torch.uint8), need

    def frames_register_ref(self, frames, window="hann"):
        """The reference side of the phase correlation (aefft_frames_register_ref): `frames` is uint8 or float32 [nref][D][Nx][Ny], nref = 1 for a
        reference the batch shares or one per image.  Channel sum, window ("hann", or "nowindow" for periodic content) and the library's R2C.
        Returns a RegisterRef holding the spectra, the window and the sizes.  The first call at a new size may allocate transform workspace."""
        what = "Context.frames_register_ref"
        nref, D, Nx, Ny = _frames4(frames, what, "[nref][D][Nx][Ny]")
        if window not in REGISTER_WINDOW:
            raise ValueError(f"{what}: window must be one of {sorted(REGISTER_WINDOW)}")
        work, need = self._register_work(Nx, Ny, nref, what)
        spec = self.empty(nref, Nx, Ny // 2 + 1, dtype=torch.complex64)
        self.check(self.L.aefft_frames_register_ref(self.h, _ptr(frames), int(_is_u8(frames)), nref, D, Nx, Ny, REGISTER_WINDOW[window], _ptr(spec), _ptr(work), need))
        return RegisterRef(spec, window, D, Nx, Ny)

    def frames_register(self, frames, ref, cutoff=0.5, min_response=0.0, scale=(1.0, 1.0), affine=False):
        """The shift of each frame against the reference by phase correlation (aefft_frames_register): `frames` uint8 or float32 [B][D][Nx][Ny],
        `ref` from frames_register_ref (one reference or B).  Returns the shifts as a uint8 device tensor [B][16] -- view it on the host with
        .cpu().numpy().view(SHIFT): dx, dy (frame cells, + when the image is the reference moved toward larger indices), response, cell --
        and with affine=True the pair (shifts, affines): an int64 device tensor (B, 6) of Q24 coefficients with the offsets dx * scale[0],
        dy * scale[1] (image pixels per frame cell), the identity where response < min_response, which Context.image_warp takes as it is.
        Nothing waits for the device."""
        B, D, Nx, Ny, sx, sy = _register_args(frames, ref, cutoff, min_response, scale)
        work, need = self._register_work(Nx, Ny, B, "Context.frames_register")
        shifts = self.empty(B, 16, dtype=torch.uint8)
        aff = self.empty(B, 6, dtype=torch.int64) if affine else None
        self.check(self.L.aefft_frames_register(self.h, _ptr(frames), int(_is_u8(frames)), B, D, Nx, Ny, REGISTER_WINDOW[ref.window], _ptr(ref.spec), ref.nref,
                                                float(cutoff), float(min_response), sx, sy, _ptr(shifts), _ptr(aff), _ptr(work), need))
        return (shifts, aff) if affine else shifts

    def image_align(self, image, ref, frame_size, cutoff=0.5, min_response=0.0, mode="linear", interp="linear", border="replicate", value=0, out=None):
        """Images put back on the reference's pixels in one call: aefft_image_resize_to_frames to frame_size = (Nx, Ny), aefft_frames_register
        against `ref` (from frames_register_ref at that size) with scale = (W / Nx, H / Ny), then aefft_image_warp_affine with the affines as
        they lie on the device.  `image` uint8 [B][H][W][D] or [H][W][D]; mode is the resize's, interp, border, value and out the warp's.
        Returns (out, shifts, affines)."""
        what = "Context.image_align"
        img, _, _ = _resize_layout(image, what)
        B, H, W, D = img.shape
        Nx, Ny = _two_ints(frame_size, what, "frame_size must be (Nx, Ny)")
        if Nx < 1 or Ny < 1 or W > 32 * Nx or H > 32 * Ny:
            raise ValueError(f"{what}: frame_size must be positive and at least (W / 32, H / 32)")
        frames = self.image_resize_to_frames(img, (Nx, Ny), mode=mode)
        shifts, aff = self.frames_register(frames, ref, cutoff=cutoff, min_response=min_response, scale=(W / Nx, H / Ny), affine=True)
        return self.image_warp(img, aff, interp=interp, border=border, value=value, out=out), shifts, aff

    def frames_degrade(self, frames, blur=0, sigma=0.0, impulse=0.0, seed=0, first_frame=0, out=None, dtype=None):
        """The degraded input of target training from the clean frames (aefft_frames_degrade), one launch: `frames` uint8 or float32
        [B][D][Nx][Ny] (float values become pixels first) -> the binomial blur of radius `blur` in 0..4 (2 blur + 1 taps per axis, edges
        replicated), additive noise of standard deviation `sigma` grey levels (an Irwin-Hall sum of six bytes: approximately normal, bounded at
        +-4.23 sigma) and salt-and-pepper impulses of probability `impulse` per element, from Philox4x32-10 keyed by `seed` and counted by
        (first_frame + b, the element's index): frame b's result depends on nothing else, so a data-parallel rank passes
        first_frame = step * global_batch + rank * B.  Returns, or fills `out` with, frames of `dtype` uint8 (rounded and clipped) or float32
        (not clipped); dtype defaults to the source's; out=frames is the in-place form (blur == 0 and the same dtype only).  All-integer
        arithmetic (include/aefft.h): the same arguments always give the same bytes.  Nothing waits for the device."""
        blur, sigma, impulse, seed, first_frame, dtype = _frames_degrade_args(frames, blur, sigma, impulse, seed, first_frame, out, dtype)
        B, D, Nx, Ny = frames.shape
        if out is None:
            out = self.empty(B, D, Nx, Ny, dtype=dtype)
        self.check(self.L.aefft_frames_degrade(self.h, _ptr(frames), int(_is_u8(frames)), _ptr(out), int(_is_u8(out)), B, D, Nx, Ny,
                                               blur, sigma, impulse, seed, first_frame))
        return out

    def image_tiles_to_frames(self, image, tile, overlap, rim=0, out=None, dtype=torch.uint8):
        """Overlapping tiles of an image as frames (aefft_image_tiles_to_frames), one launch: `image` is a uint8 device tensor [B][H][W][D] (or
        [H][W][D]) laid out as image_resize_to_frames takes it; tile = (Nx, Ny), the net's frame size; `overlap` the pixels two neighbouring
        tiles share and `rim` the pixels at each tile edge that the blend never uses, each an int or an (x, y) pair (tile_plan gives the grid).
        Beyond the image's edge the tiles hold reflected pixels (the edge pixel not repeated).  Returns, or fills `out` with, the frames
        [B * ntx * nty][D][Nx][Ny] of `dtype` uint8 or float32, image-major, then tile row, then tile column.  Nothing waits for the device."""
        img, pitch, stride, desc, shape, dtype = _image_tiles_args(image, tile, overlap, rim, out, dtype)
        if out is None:
            out = self.empty(*shape, dtype=dtype)
        self.check(self.L.aefft_image_tiles_to_frames(self.h, _ptr(img), pitch, stride, C.byref(desc), _ptr(out), int(_is_u8(out)), img.shape[0], img.shape[3]))
        return out

    def frames_tiles_to_image(self, frames, size, overlap, rim=0, out=None):
        """Tile frames blended back into images (aefft_frames_tiles_to_image), one launch, the inverse of image_tiles_to_frames: `frames` is
        uint8 or float32 [B * ntx * nty][D][Nx][Ny] (float values become pixels first); size = (W, H); `overlap` and `rim` as given to the
        gather.  Each pixel is the integer-weighted mean of the one, two or four tiles whose kept area covers it: linear ramps across the
        overlap minus the rims, so unchanged tiles give back the image's bytes.  Returns, or fills `out` with, the uint8 image rows
        [B][H][W][D]; `out` may be row-padded or a region of interest (bytes outside it are not written).  Nothing waits for the device."""
        desc, shape = _frames_tiles_args(frames, size, overlap, rim, out)
        if out is None:
            out = self.empty(*shape, dtype=torch.uint8)
        img, pitch, stride = _resize_layout(out, "Context.frames_tiles_to_image")
        self.check(self.L.aefft_frames_tiles_to_image(self.h, _ptr(frames), int(_is_u8(frames)), C.byref(desc), _ptr(img), pitch, stride, shape[0], shape[3]))
        return out

    def yuv_to_image(self, planes, fmt, matrix="bt601", order="bgr", out=None):
        """Colour conversion on the device (aefft_yuv_to_image): `planes` is a tuple of uint8 device tensors -- fmt "nv12": (y [B][H][W],
        uv [B][Hc][Wc][2]); "i420": (y, u [B][Hc][Wc], v); "yuyv": (yuyv [B][H][W/2][4],); unbatched tensors too -- each contiguous or a view with a
        row pitch and any sufficient batch stride (two views into one decoder surface work; ValueError otherwise).  matrix "bt601", "bt709"
        (limited range) or "jpeg" (601 full range); order "bgr", "rgb" (D = 3) or "gray" (D = 1, the chroma planes are not read).  Chroma is
        replicated (nearest).  Returns, or fills `out` with, the uint8 image rows [B][H][W][D]; `out` may be a row-padded view or a region of
        interest.  All-integer arithmetic (include/aefft.h).  One launch, nothing waits for the device."""
        what = "Context.yuv_to_image"
        desc, B, W, H, D, keep = _yuv_source(planes, fmt, matrix, order, what)      # (keep: the views the descriptor points into)
        if out is None:
            out = self.empty(B, H, W, D, dtype=torch.uint8)
        img, pitch, stride = _resize_layout(out, what)
        if tuple(img.shape) != (B, H, W, D):
            raise ValueError(f"{what}: out must have shape {(B, H, W, D)}")
        self.check(self.L.aefft_yuv_to_image(self.h, C.byref(desc), YUV_ORDERS[order], _ptr(img), pitch, stride, B))
        return out

    def raw_to_image(self, raw, pattern, bits=8, packed=False, black=0, white=None, gains=(1, 1, 1), method="mhc", order="bgr", ccm=None, lut=None, out=None):
        """Raw sensor data to 8-bit images on the device (aefft_raw_to_image), one launch: `raw` is a uint8 device tensor [B][H][W] (or [H][W])
        of 8-bit samples, with packed=True the bytes [B][H][ceil(W * bits / 8)] of GenICam 10p / 12p rows, or an int16 / uint16 tensor [B][H][W]
        with the sample in the low `bits` (9..16) bits; contiguous or a view with a row pitch and any sufficient batch stride.  `pattern` is
        GenICam's name of the mosaic -- "rggb" (BayerRG), "grbg", "gbrg", "bggr" -- or "mono"; `black` and `white` (None: 2**bits - 1) the sensor
        levels mapped to 0 and 255, `gains` the white balance (R, G, B; mono: one number or the first), applied before the demosaic "mhc"
        (Malvar-He-Cutler, 5 x 5) or "bilinear"; `ccm` an optional 3 x 3 colour matrix (out = ccm * (R, G, B)); `lut` an optional 4096-byte
        table indexed in sixteenths of a linear grey level (gamma_lut, srgb_lut: a numpy array, uploaded here, or a uint8 device tensor).
        Returns, or fills `out` with, the uint8 image rows [B][H][W][D], D = 3 in `order` "bgr" or "rgb", D = 1 for mono; `out` may be a
        row-padded view or a region of interest.  All-integer arithmetic (include/aefft.h).  Nothing waits for the device."""
        what = "Context.raw_to_image"
        desc, B, W, H, D, keep = _raw_source(raw, pattern, bits, packed, black, white, gains, method, order, ccm, what)
        if lut is not None:
            if isinstance(lut, np.ndarray):
                if lut.dtype != np.uint8 or lut.size != 4096:
                    raise ValueError(f"{what}: lut must hold 4096 uint8 entries")
                cache = self.__dict__.setdefault("_raw_luts", {})              # (uploaded once a table and kept: the launch may still be queued on return)
                key = lut.tobytes()
                if key not in cache:
                    cache[key] = torch.as_tensor(np.frombuffer(key, dtype=np.uint8).copy(), device=f"cuda:{self.device}")
                lut = cache[key]
            elif not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or lut.numel() != 4096 or not lut.is_contiguous():
                raise ValueError(f"{what}: lut must be a numpy array or a contiguous uint8 device tensor of 4096 entries")
            desc.lut_d = lut.data_ptr()
        if out is None:
            out = self.empty(B, H, W, D, dtype=torch.uint8)
        img, pitch, stride = _resize_layout(out, what)
        if tuple(img.shape) != (B, H, W, D):
            raise ValueError(f"{what}: out must have shape {(B, H, W, D)}")
        self.check(self.L.aefft_raw_to_image(self.h, C.byref(desc), YUV_ORDERS.get(order, 0), _ptr(img), pitch, stride, B))
        return out

    def yuv_resize_to_frames(self, planes, fmt, size, matrix="bt601", order="bgr", mode="linear", out=None, dtype=torch.uint8):
        """Colour conversion + resize + ImageToSpin_C on the device in one launch (aefft_yuv_resize_to_frames): `planes`, `fmt`, `matrix` and
        `order` as for yuv_to_image; size = (Nx, Ny) and mode as for image_resize_to_frames.  Returns, or fills `out` with, the planar frames
        [B][D][Nx][Ny] of `dtype` uint8 or float32 -- bit for bit yuv_to_image followed by image_resize_to_frames, without the image in
        between.  Nothing waits for the device."""
        what = "Context.yuv_resize_to_frames"
        desc, B, W, H, D, keep = _yuv_source(planes, fmt, matrix, order, what)      # (keep: the views the descriptor points into)
        if mode not in RESIZE_MODES:
            raise ValueError(f"{what}: mode must be one of {sorted(RESIZE_MODES)}")
        Nx, Ny = _two_ints(size, what, "size must be (Nx, Ny)")
        if out is None:
            if dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"{what}: dtype must be torch.uint8 or torch.float32")
            if Nx < 1 or Ny < 1:
                raise ValueError(f"{what}: size must be positive")
            out = self.empty(B, D, Nx, Ny, dtype=dtype)
        elif out.dtype not in (torch.uint8, torch.float32) or tuple(out.shape) != (B, D, Nx, Ny) or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous uint8 or float32 tensor of shape {(B, D, Nx, Ny)}")
        self.check(self.L.aefft_yuv_resize_to_frames(self.h, C.byref(desc), YUV_ORDERS[order], RESIZE_MODES[mode], _ptr(out), int(_is_u8(out)), B, Nx, Ny))
        return out

    def _yuv_out_planes(self, fmt, matrix, order, B, W, H, D, out, what):
        """(the planes to return, the YuvDst over them, the views it points into): `out`, or fresh contiguous planes"""
        dst, keep = _yuv_dest(fmt, matrix, order, B, W, H, D, out, what)
        if dst is None:
            out = tuple(self.empty(*s, dtype=torch.uint8) for s in yuv_plane_shapes(fmt, B, W, H))
            dst, keep = _yuv_dest(fmt, matrix, order, B, W, H, D, out, what)
        return out, dst, keep

    def image_to_yuv(self, image, fmt, matrix="bt601", order="bgr", out=None):
        """Colour conversion on the device, the way out (aefft_image_to_yuv), the mirror of yuv_to_image: `image` is a uint8 device tensor
        [B][H][W][D] (or [H][W][D]) laid out as image_resize_to_frames takes it, D = 3 for order "bgr" / "rgb" and 1 for "gray" (every chroma sample
        128).  Returns, or fills `out` with, the tuple of plane tensors yuv_to_image takes -- fmt "nv12": (y [B][H][W], uv [B][Hc][Wc][2]); "i420":
        (y, u [B][Hc][Wc], v); "yuyv": (yuyv [B][H][W/2][4],), W even -- `out` planes may be strided views into one encoder surface.  Luma per
        pixel, chroma the rounded box average of its live pixels; all-integer arithmetic (include/aefft.h).  One launch, nothing waits for the
        device."""
        what = "Context.image_to_yuv"
        img, pitch, stride = _resize_layout(image, what)
        B, H, W, D = img.shape
        out, dst, keep = self._yuv_out_planes(fmt, matrix, order, B, W, H, D, out, what)      # (keep: the views the descriptor points into)
        self.check(self.L.aefft_image_to_yuv(self.h, _ptr(img), pitch, stride, YUV_ORDERS[order], C.byref(dst), B))
        return out

    def frames_resize_to_yuv(self, frames, size, fmt, matrix="bt601", order="bgr", mode="linear", out=None):
        """SpinToImage_C + resize + colour conversion on the device in one launch (aefft_frames_resize_to_yuv): `frames` uint8 or float32
        [B][D][Nx][Ny] as frames_resize_to_image takes them, size = (W, H) and mode as there; fmt, matrix, order and `out` as for image_to_yuv.
        Returns, or fills `out` with, the plane tensors -- bit for bit frames_resize_to_image followed by image_to_yuv, without the image in
        between.  Nothing waits for the device."""
        what = "Context.frames_resize_to_yuv"
        B, D, Nx, Ny = _frames4(frames, what)
        if mode not in RESIZE_MODES:
            raise ValueError(f"{what}: mode must be one of {sorted(RESIZE_MODES)}")
        W, H = _two_ints(size, what, "size must be (W, H)")
        out, dst, keep = self._yuv_out_planes(fmt, matrix, order, B, W, H, D, out, what)      # (keep: the views the descriptor points into)
        self.check(self.L.aefft_frames_resize_to_yuv(self.h, _ptr(frames), int(_is_u8(frames)), Nx, Ny, RESIZE_MODES[mode], YUV_ORDERS[order], C.byref(dst), B))
        return out

    def set_flags(self, *names):
        """Development switches (include/aefft.h AEFFT_F_*), by name without the prefix; no names = defaults."""
        v = 0
        for nme in names:
            if nme:
                v |= FLAGS[nme.replace("AEFFT_", "").replace("F_", "")]
        self.check(self.L.aefft_ctx_set_flags(self.h, v))

    def get_flags(self):
        return int(self.L.aefft_ctx_get_flags(self.h))

    # ---- profiling ----
    def prof_enable(self, on=True):
        self.check(self.L.aefft_prof_enable(self.h, 1 if on else 0))

    def prof_reset(self):
        self.check(self.L.aefft_prof_reset(self.h))

    def prof_read(self):
        out = {}
        for kid in range(self.L.aefft_prof_count()):
            n, ms, by = C.c_long(), C.c_double(), C.c_double()
            self.check(self.L.aefft_prof_read(self.h, kid, C.byref(n), C.byref(ms), C.byref(by)))
            out[self.L.aefft_prof_name(kid).decode()] = dict(launches=n.value, ms=ms.value, bytes=by.value)
        return out


class Net:
    """aefft_net: resident batched autoencoder (autoenc_fft / backprop_fft semantics)."""

    def __init__(self, ctx, D, Nx, Ny, maps, Nk, scale, batch, Nl=None, smooth_sizes=False, spatial=False, operator_form=False):
        """smooth_sizes: also take Nx, Ny with prime factors 3 and 5 (640 x 480, ...; aefft_net_create_ex with
        AEFFT_NET_SMOOTH_SIZES) -- such a net trains in the per-frame form, unless
        operator_form (AEFFT_NET_SMOOTH_OPFORM, with smooth_sizes): it trains in the operator form where it meets that form's rules
        (step_form() reports the form it runs in); no effect on a power-of-two net, on a spatial net or without smooth_sizes.
        spatial: the coordinate-space mode (Pool / Conv_gpu / backprop_gpu; aefft_net_create_ex with AEFFT_NET_SPATIAL): any frame size,
        every scale dividing its input grid exactly; step_apply's del0 is backprop_gpu's delmax and the MSE tail is this step's."""
        self.ctx, self.L = ctx, ctx.L
        self.D, self.Nx, self.Ny, self.B = D, Nx, Ny, batch
        self.spatial = bool(spatial)
        self.maps = list(maps); self.npairs = len(self.maps)
        self.Nk = [Nk] * self.npairs if isinstance(Nk, int) else list(Nk)
        self.Nl = list(self.Nk) if Nl is None else ([Nl] * self.npairs if isinstance(Nl, int) else list(Nl))
        self.scale = [scale] * self.npairs if isinstance(scale, int) else list(scale)
        arr = lambda v: (C.c_int * self.npairs)(*v)
        self._keep = [arr(self.maps), arr(self.Nk), arr(self.Nl), arr(self.scale)]
        d = NetDesc(D, Nx, Ny, self.npairs, *self._keep, batch)
        h = C.c_void_p()
        if smooth_sizes or spatial or operator_form:
            opts = (NET_SMOOTH_SIZES if smooth_sizes else 0) | (NET_SPATIAL if spatial else 0) | (NET_SMOOTH_OPFORM if operator_form else 0)
            ctx.check(self.L.aefft_net_create_ex(ctx.h, C.byref(d), opts, C.byref(h)))
        else:
            ctx.check(self.L.aefft_net_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h
        # per-pair geometry
        self.dims = []
        dD, nx, ny = D, Nx, Ny
        for l in range(self.npairs):
            nx //= self.scale[l]; ny //= self.scale[l]
            self.dims.append(dict(dD=dD, dM=self.maps[l], Nx=nx, Ny=ny, Nk=self.Nk[l], Nl=self.Nl[l]))
            dD = self.maps[l]

    def close(self):
        if getattr(self, "h", None):
            self.L.aefft_net_destroy(self.h)
            self.h = None

    def __del__(self):
        if _exiting:      # interpreter shutdown: the HIP runtime may already be gone; the process frees everything
            return
        try:
            self.close()
        except Exception:
            pass

    def set_pair(self, l, c, b, f, p):
        a = [np.ascontiguousarray(v, np.float32) for v in (c, b, f, p)]
        g = self.dims[l]
        assert a[0].shape == (g["dM"], g["dD"], g["Nk"], g["Nl"]) and a[2].shape == (g["dD"], g["dM"], g["Nk"], g["Nl"])
        assert a[1].shape == (g["dM"],) and a[3].shape == (g["dD"],)
        self.ctx.check(self.L.aefft_net_set_pair(self.h, l, *[_hptr(v) for v in a]))

    def get_pair(self, l):
        g = self.dims[l]
        c = np.empty((g["dM"], g["dD"], g["Nk"], g["Nl"]), np.float32); f = np.empty((g["dD"], g["dM"], g["Nk"], g["Nl"]), np.float32)
        b = np.empty(g["dM"], np.float32); p = np.empty(g["dD"], np.float32)
        self.ctx.check(self.L.aefft_net_get_pair(self.h, l, _hptr(c), _hptr(b), _hptr(f), _hptr(p)))
        return c, b, f, p

    def store_spectra(self, l):
        g = self.dims[l]
        nyr = g["Ny"] // 2 + 1
        Cs = np.empty((g["dM"], g["dD"], g["Nx"], nyr), np.complex64); Fs = np.empty((g["dD"], g["dM"], g["Nx"], nyr), np.complex64)
        self.ctx.check(self.L.aefft_net_store_spectra(self.h, l, _hptr(Cs), _hptr(Fs)))
        return Cs, Fs

    def load_spectra(self, l, Cs, b, Fs, p):
        a = [np.ascontiguousarray(Cs, np.complex64), np.ascontiguousarray(b, np.float32),
             np.ascontiguousarray(Fs, np.complex64), np.ascontiguousarray(p, np.float32)]
        self.ctx.check(self.L.aefft_net_load_spectra(self.h, l, *[_hptr(v) for v in a]))

    def forward(self, frames, recon=None):
        fn = self.L.aefft_net_forward_u8 if _is_u8(frames) else self.L.aefft_net_forward
        self.ctx.check(fn(self.h, _ptr(frames), _ptr(recon)))
        return recon

    def infer(self, frames, recon=None, hidden_pair=None, hidden=None):
        """Frozen-weight inference over the batch (aefft_net_infer): the reconstruction into `recon` and/or the hidden layer of pair
        `hidden_pair` (layer 2*hidden_pair+2, float32 [B][dM][Nx_l][Ny_l]) into `hidden`, from the current weights.  uint8 `frames` are read as
        8-bit pixels; a uint8 `recon` receives clamp(round(v), 0, 255) (SpinToImage_C).  Operator-form nets (step_form) evaluate the layers once
        per weight set.  Returns (recon, hidden)."""
        if hidden is not None and hidden_pair is None:
            raise ValueError("Net.infer: hidden given without hidden_pair")
        hp = -1 if hidden_pair is None else int(hidden_pair)
        self.ctx.check(self.L.aefft_net_infer(self.h, _ptr(frames), int(_is_u8(frames)), _ptr(recon), int(_is_u8(recon)), hp, _ptr(hidden)))
        return recon, hidden

    def infer_tiled(self, image, overlap, rim=0, out=None):
        """Frozen-weight inference at the image's own resolution: `image` is a uint8 device tensor [B][H][W][D] of any size, cut into overlapping
        tiles of the net's (Nx, Ny) (Context.image_tiles_to_frames), reconstructed by aefft_net_infer in chunks of the net's batch (8-bit in,
        8-bit out) and blended into `out`, uint8 [B][H][W][D] (Context.frames_tiles_to_image).  `rim` should cover the summed kernel reach of the
        net, whose circular convolution contaminates that much of every tile's edge; `overlap` is 2 * rim plus the ramp the seam is blended
        over.  The tile buffer is rounded up to a multiple of the batch; the padding frames are zero and ignored.  An FFT net only
        (ValueError on a spatial net).  Nothing waits for the device.  Returns `out`."""
        what = "Net.infer_tiled"
        if self.spatial:
            raise ValueError(f"{what}: tiled inference serves the FFT net (its circular convolution is what the rim is for), not a spatial net")
        if image.dim() != 4:
            raise ValueError(f"{what}: the image must be a uint8 tensor [B][H][W][D]")
        img, pitch, stride, desc, shape, _ = _image_tiles_args(image, (self.Nx, self.Ny), overlap, rim, None, torch.uint8)
        B, H, W, D = img.shape
        if D != self.D:
            raise ValueError(f"{what}: the image has {D} channels, the net {self.D}")
        if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, D)):
            raise ValueError(f"{what}: out must be a uint8 tensor of shape {(B, H, W, D)}")
        T = shape[0]
        Tp = -(-T // self.B) * self.B
        tiles = torch.zeros(Tp, D, self.Nx, self.Ny, dtype=torch.uint8, device=image.device)
        recon = torch.empty_like(tiles)
        self.ctx.image_tiles_to_frames(img, (self.Nx, self.Ny), overlap, rim, out=tiles[:T])
        for k in range(0, Tp, self.B):
            self.infer(tiles[k:k + self.B], recon[k:k + self.B])
        return self.ctx.frames_tiles_to_image(recon[:T], (W, H), overlap, rim, out=out)

    def score_tiled(self, image, overlap, rim=0, tile=16, metric="mse", target=None, map=None, score=None, out=None):
        """Reconstruction error at the image's own resolution: infer_tiled(image, overlap, rim) into `out`, then Context.image_compare_map of
        `target` (the image itself when None) against `out` on cells_for_tile(W, H, tile) -- cells of about `tile` pixels a side, an int or an
        (x, y) pair in 1..64; metric "mse" or "ssim".  `map`, `score` and `out` are allocated when None; score=False skips the score.  An FFT
        net only (ValueError on a spatial net).  Nothing waits for the device.  Returns (map, score, out)."""
        out = self.infer_tiled(image, overlap, rim, out=out)          # (its checks are this call's: an FFT net, a uint8 image [B][H][W][D])
        cells = cells_for_tile(out.shape[2], out.shape[1], tile)
        map, score = self.ctx.image_compare_map(image if target is None else target, out, cells, metric, map=map, score=score)
        return map, score, out

    def detect_tiled(self, image, overlap, rim=0, tile=16, metric="mse", lo=None, hi=None, ref=None, connectivity=8, min_area=1, max_regions=256,
                     target=None, out=None):
        """Detections at the image's own resolution: score_tiled(image, overlap, rim, tile, metric, target, out=out) without the score, then
        Context.map_regions of its map with sense "below" when metric == "ssim" and "above" otherwise (`lo` is required; hi, ref, connectivity,
        min_area and max_regions as there).  Context.region_pixels / region_pixels(region, cells_for_tile(W, H, tile), W, H) carries a box to
        pixels.  An FFT net only.  Nothing waits for the device.  Returns (labels, regions, count, map, out)."""
        if lo is None:
            raise ValueError("Net.detect_tiled: lo (the threshold) is required")
        map, _, out = self.score_tiled(image, overlap, rim, tile=tile, metric=metric, target=target, score=False, out=out)
        labels, regions, count = self.ctx.map_regions(map, lo, hi, ref=ref, sense="below" if metric == "ssim" else "above", connectivity=connectivity,
                                                      min_area=min_area, max_regions=max_regions)
        return labels, regions, count, map, out

    def calibrate_tiled(self, image, overlap, rim=0, tile=16, metric="mse", state=None, target=None):
        """Nominal footage into a calibration state: score_tiled(image, overlap, rim, tile, metric, target) without the score, then
        Context.map_stats_update of its map into `state` (Context.map_stats of the map's grid when None).  Context.map_stats_finish(state,
        cells_for_tile(W, H, tile), ...) then gives the `ref` detect_tiled takes.  An FFT net only.  Nothing waits for the device.  Returns
        (state, map)."""
        map, _, _ = self.score_tiled(image, overlap, rim, tile=tile, metric=metric, target=target, score=False)
        if state is None:
            state = self.ctx.map_stats(map.shape[1], map.shape[2])
        self.ctx.map_stats_update(state, map)
        return state, map

    def score(self, frames, score=None, recon=None):
        """Per-frame reconstruction error under the current weights (aefft_net_score): score[b] = mean over the frame's D*Nx*Ny pixels of
        (x - r)^2, r the float32 reconstruction Net.infer would write.  uint8 `frames` are read as 8-bit pixels.  `score` (float32 [B]) is
        allocated when None; `recon` (float32 [B][D][Nx][Ny], optional) receives the reconstruction from the same launch -- the spatial net
        and the chirp-z transforms need it.  Nothing waits for the device.  Returns (score, recon)."""
        if score is None:
            score = self.ctx.empty(self.B)
        self.ctx.check(self.L.aefft_net_score(self.h, _ptr(frames), int(_is_u8(frames)), _ptr(score), _ptr(recon)))
        return score, recon

    def score_map(self, frames, tile, map=None, score=None, recon=None):
        """Per-tile reconstruction error under the current weights (aefft_net_score_map): map[b][I][J] = mean over the D channels and the
        tile x tile pixels of tile (I, J) of (x - r)^2, r the float32 reconstruction Net.infer would write.  `tile` is 8, 16, 32 or 64 and divides
        Nx and Ny.  uint8 `frames` are read as 8-bit pixels.  `map` (float32 [B][Nx/tile][Ny/tile]) and `score` (float32 [B], the mean of the
        frame's map entries) are allocated when None; `recon` (float32 [B][D][Nx][Ny], optional) receives the reconstruction from the same
        launch -- the spatial net and the chirp-z transforms need it.  Nothing waits for the device.  Returns (map, score, recon)."""
        tile = int(tile)
        if map is None:
            t = max(tile, 1)                  # (a tile the library refuses still gets a buffer: the error is the library's)
            map = self.ctx.empty(self.B, max(self.Nx // t, 1), max(self.Ny // t, 1))
        if score is None:
            score = self.ctx.empty(self.B)
        self.ctx.check(self.L.aefft_net_score_map(self.h, _ptr(frames), int(_is_u8(frames)), tile, _ptr(map), _ptr(score), _ptr(recon)))
        return map, score, recon

    def score_target(self, frames, targets, score=None, recon=None):
        """Net.score against a target (aefft_net_score_target): the net reads `frames`, score[b] = mean of (t - r)^2 with t the pixels of
        `targets` (float32 or uint8 [B][D][Nx][Ny], on its own) -- the validation number of a net trained by step_grad_target.
        Returns (score, recon)."""
        if score is None:
            score = self.ctx.empty(self.B)
        self.ctx.check(self.L.aefft_net_score_target(self.h, _ptr(frames), int(_is_u8(frames)), _ptr(targets), int(_is_u8(targets)), _ptr(score), _ptr(recon)))
        return score, recon

    def score_map_target(self, frames, targets, tile, map=None, score=None, recon=None):
        """Net.score_map against a target (aefft_net_score_map_target): the net reads `frames`, the map holds the block means of (t - r)^2 with
        t the pixels of `targets` (float32 or uint8 [B][D][Nx][Ny], on its own).  Returns (map, score, recon)."""
        tile = int(tile)
        if map is None:
            t = max(tile, 1)
            map = self.ctx.empty(self.B, max(self.Nx // t, 1), max(self.Ny // t, 1))
        if score is None:
            score = self.ctx.empty(self.B)
        self.ctx.check(self.L.aefft_net_score_map_target(self.h, _ptr(frames), int(_is_u8(frames)), _ptr(targets), int(_is_u8(targets)), tile,
                                                         _ptr(map), _ptr(score), _ptr(recon)))
        return map, score, recon

    def ssim_map(self, frames, tile, targets=None, data_range=255.0, map=None, score=None, recon=None):
        """Block SSIM of the reconstruction under the current weights (aefft_net_ssim_map): map[b][I][J] = mean over the D channels of the SSIM
        of window (I, J) -- tile x tile pixels, uniform weights, population statistics, C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range --
        between the reference (`targets`, or the frames when None) and r, the float32 reconstruction Net.infer would write.  `tile` is 8, 16, 32
        or 64 and divides Nx and Ny.  `map` (float32 [B][Nx/tile][Ny/tile]) and `score` (float32 [B], the mean of the frame's map entries) are
        allocated when None; `recon` (optional) receives the reconstruction from the same launch -- the spatial net and the chirp-z transforms
        need it.  The first call of a net allocates the strip buffer.  Returns (map, score, recon)."""
        tile = int(tile)
        if map is None:
            t = max(tile, 1)
            map = self.ctx.empty(self.B, max(self.Nx // t, 1), max(self.Ny // t, 1))
        if score is None:
            score = self.ctx.empty(self.B)
        self.ctx.check(self.L.aefft_net_ssim_map(self.h, _ptr(frames), int(_is_u8(frames)), _ptr(targets), int(_is_u8(targets)), tile, float(data_range),
                                                 _ptr(map), _ptr(score), _ptr(recon)))
        return map, score, recon

    def decode(self, code, hidden_pair, recon):
        """The reconstruction from a stored hidden layer (aefft_net_decode): `code` is float32 [B][dM][Nx_l][Ny_l] of pair `hidden_pair`, as
        Net.infer writes `hidden`; a uint8 `recon` receives clamp(round(v), 0, 255) (SpinToImage_C).  Operator-form nets (step_form) form the
        decoding operator once per weight set and pair.  No frame stands behind the call: get_layer(s) raise until the next forward.
        Returns recon."""
        self.ctx.check(self.L.aefft_net_decode(self.h, int(hidden_pair), _ptr(code), _ptr(recon), int(_is_u8(recon))))
        return recon

    def get_layer(self, layer):
        ch, nx, ny = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.L.aefft_net_get_layer(self.h, layer, None, C.byref(ch), C.byref(nx), C.byref(ny)))
        out = self.ctx.empty(self.B, ch.value, nx.value, ny.value)
        self.ctx.check(self.L.aefft_net_get_layer(self.h, layer, _ptr(out), None, None, None))
        return out

    def get_layers(self):
        """every layer 0..4L of the last forward in one call: list of torch views into one packed buffer"""
        nl = 4 * self.npairs + 1
        offs = (C.c_size_t * (nl + 1))()
        self.ctx.check(self.L.aefft_net_layers_layout(self.h, offs))
        buf = self.ctx.empty(int(offs[nl]))
        self.ctx.check(self.L.aefft_net_get_layers(self.h, _ptr(buf)))
        out = []
        for l in range(nl):
            ch, nx, ny = C.c_int(), C.c_int(), C.c_int()
            self.ctx.check(self.L.aefft_net_get_layer(self.h, l, None, C.byref(ch), C.byref(nx), C.byref(ny)))
            out.append(buf[int(offs[l]):int(offs[l + 1])].view(self.B, ch.value, nx.value, ny.value))
        return out

    def train_pair(self, l, n_iter, del0, maxdiff=0, sym=0):
        mse = np.zeros(n_iter + 1, np.float32)
        self.ctx.check(self.L.aefft_net_train_pair(self.h, l, n_iter, del0, maxdiff, sym, _hptr(mse)))
        return mse

    def set_input_ready(self, on=True):
        """Frames given to step_grad are complete when the call is made: their R2C may run ahead on a side stream."""
        self.ctx.check(self.L.aefft_net_set_input_ready(self.h, 1 if on else 0))

    def step_grad(self, frames, recon=None):
        """frames: float32 [B][D][Nx][Ny], or uint8 of the same shape (8-bit pixels: aefft_net_step_grad_u8, converted by the input transform)."""
        fn = self.L.aefft_net_step_grad_u8 if _is_u8(frames) else self.L.aefft_net_step_grad
        self.ctx.check(fn(self.h, _ptr(frames), _ptr(recon)))

    def step_grad_target(self, frames, targets, recon=None):
        """step_grad toward a target (aefft_net_step_grad_target): pair 0's expected output is the spectrum of `targets` instead of the frames'
        own -- denoising, deblurring, restoration.  frames, targets: float32 or uint8 [B][D][Nx][Ny], each on its own (8-bit pixels convert on
        load).  The following step_apply is the usual one; pair 0's post-update MSE is then taken against the target.  The first call of a
        net allocates the target's workspaces."""
        self.ctx.check(self.L.aefft_net_step_grad_target(self.h, _ptr(frames), int(_is_u8(frames)), _ptr(targets), int(_is_u8(targets)), _ptr(recon)))

    def grad_buffer(self):
        """torch view of the packed gradient buffer (for torch.distributed.all_reduce)."""
        p, n = C.c_void_p(), C.c_size_t()
        self.ctx.check(self.L.aefft_net_grad_buffer(self.h, C.byref(p), C.byref(n)))
        t = self.ctx.torch
        if not hasattr(self, "_gradview") or self._gradview[0] != p.value:
            iface = {"shape": (n.value,), "typestr": "<f4", "data": (p.value, False), "version": 2, "strides": None}
            holder = type("_Raw", (), {"__cuda_array_interface__": iface})()
            self._gradview = (p.value, t.as_tensor(holder, device=f"cuda:{self.ctx.device}"))
        return self._gradview[1]

    def mse_prev_global(self):
        """torch view of the L floats behind the packed buffer: the global-batch post-update MSE per pair of the step BEFORE the last
        aefft_net_step_apply (the reduced tail of the last all-reduce times grad_scale, saved by step_apply itself; include/aefft.h)."""
        p, n = C.c_void_p(), C.c_size_t()
        self.ctx.check(self.L.aefft_net_grad_buffer(self.h, C.byref(p), C.byref(n)))
        t = self.ctx.torch
        if not hasattr(self, "_prevview") or self._prevview[0] != p.value:
            iface = {"shape": (self.npairs,), "typestr": "<f4", "data": (p.value + 4 * n.value, False), "version": 2, "strides": None}
            holder = type("_Raw", (), {"__cuda_array_interface__": iface})()
            self._prevview = (p.value, t.as_tensor(holder, device=f"cuda:{self.ctx.device}"))
        return self._prevview[1]

    def step_form(self):
        """which form the next training step runs in: "per_frame", "operator", "operator_chain" or, on a spatial net, "spatial"
        (aefft_net_step_form)"""
        return ("per_frame", "operator", "operator_chain", "spatial")[self.L.aefft_net_step_form(self.h)]

    def tail_route(self):
        """which step code the last tail launch ran: "static" (compile-time step table for the net's channel counts), "generic", or None before
        the first one (aefft_net_tail_route)"""
        return (None, "generic", "static")[self.L.aefft_net_tail_route(self.h)]

    def step_apply(self, del0, maxdiff=0, sym=0, grad_scale=1.0, mse=None):
        self.ctx.check(self.L.aefft_net_step_apply(self.h, del0, maxdiff, sym, grad_scale, _ptr(mse)))

    def last_mse(self, mse=None):
        """per-pair post-update MSE of the last step_apply (aefft_net_last_mse): sums them now if step_apply(mse=None) left that to the next step"""
        if mse is None:
            mse = self.ctx.empty(self.npairs)
        self.ctx.check(self.L.aefft_net_last_mse(self.h, _ptr(mse)))
        return mse

    def reset_momentum(self):
        self.ctx.check(self.L.aefft_net_reset_momentum(self.h))

    def set_inertia(self, alpha):
        """inertia weight of backprop_gpu's update on a spatial net (default 0.9; aefft_net_set_inertia)"""
        self.ctx.check(self.L.aefft_net_set_inertia(self.h, alpha))
