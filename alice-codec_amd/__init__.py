"""alice_codec_amd -- host-side mirror of the ALICE-Codec encode/decode API over the
MI355X (gfx950) C-ABI library ``libalice_codec.so``.

The names follow the reference's public surface (Rust ``src/pipeline.rs``,
``src/wavelet.rs``, ``src/quant.rs``, ``src/rans.rs`` and its PyO3 module
``src/python.rs:408-482``): ``FrameEncoder``, ``FrameDecoder``, ``EncodedChunk``,
``WaveletType``, ``Wavelet1D/2D/3D``, ``Quantizer``, ``FastQuantizer``,
``to_symbols`` / ``from_symbols`` / ``build_histogram``, ``FrequencyTable``,
``RansEncoder`` / ``RansDecoder``.  Every call goes through the C ABI declared in
``include/alice_codec.h`` and runs on the GPU.  There is no CPU fallback: when the
library is missing or no HIP device is usable this module raises.
"""
from __future__ import annotations

import ctypes as C
import weakref
import enum
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# Kernels of HIP streams that share a hardware queue run one after the other, the runtime creates 4 queues by default, and
# a chain kernel runs for seconds: host threads calling encode / decode concurrently need more (csrc/codec.hip,
# widen_hw_queues_once).  The library asks for 8 itself, but in a Python process torch usually initialises HIP first -- so
# ask here, at import, before anything has touched the device.  An existing setting is kept.
if not os.environ.get("ALICE_CODEC_KEEP_HW_QUEUES"):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

# ALICE_CODEC_LIB: developer override (A/B runs of two builds of the library); the product loads the in-tree build
LIB_PATH = os.environ.get("ALICE_CODEC_LIB") or os.path.join(_HERE, "libalice_codec.so")

VERSION = "0.1.2"
DEFAULT_CHUNK_SIZE = 64  # reference src/lib.rs:110


class WaveletType(enum.IntEnum):  # reference src/pipeline.rs:34-41
    Cdf53 = 0
    Cdf97 = 1
    Haar = 2


PREVIEWS_MAX_ITEMS = 1024          # ALICE_PREVIEWS_MAX_ITEMS
PREVIEWS_NO_ITEM = 0xFFFFFFFF      # *bad_item of a refusal that is no item's


class PreviewItem(C.Structure):
    """alice_codec_preview_item of include/alice_codec.h"""
    _fields_ = [("alc", C.c_void_p), ("len", C.c_uint64), ("first", C.c_uint32), ("count", C.c_uint32), ("rgb_out", C.c_void_p)]


RECTS_MAX_ITEMS = 1024             # ALICE_RECTS_MAX_ITEMS


class RectItem(C.Structure):
    """alice_codec_rect_item of include/alice_codec.h (64 bytes)"""
    _fields_ = [("alc", C.c_void_p), ("len", C.c_uint64), ("first", C.c_uint32), ("count", C.c_uint32), ("x", C.c_uint32),
                ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("rgb_out", C.c_void_p), ("row_pitch", C.c_uint64),
                ("frame_pitch", C.c_uint64)]


class CodecError(Exception):
    """Mirror of the reference ``CodecError`` (src/error.rs:12-23)."""

    NAMES = {
        1: "InvalidBufferSize", 2: "InvalidDimensions", 3: "DimensionOverflow", 4: "InvalidBitstream",
        5: "InvalidQuantStep", 6: "ReferenceDiverges", 7: "OutOfMemory", 8: "DeviceError",
        9: "NullArgument", 10: "Internal",
    }

    def __init__(self, code: int, message: str = ""):
        self.code = code
        self.kind = self.NAMES.get(code, f"Error{code}")
        super().__init__(f"{self.kind}: {message}" if message else self.kind)


_u8p = C.POINTER(C.c_uint8)
_i16p = C.POINTER(C.c_int16)
_u16p = C.POINTER(C.c_uint16)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)

_lib = None


def _preload_hip_runtime() -> None:
    """One process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so.7 / libhsa-runtime64 next to libtorch; libalice_codec.so is linked against
    the same SONAME.  If the system copy were loaded first and torch's afterwards, two HSA
    runtimes would fight over the device ("No HIP GPUs are available").  When torch is
    installed, load its copy first so both bind to it, whatever the import order.  Set
    ALICE_CODEC_HIP_RUNTIME=system to skip this (pure C/C++ hosts never need it)."""
    if os.environ.get("ALICE_CODEC_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    import sys
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if "torch" not in sys.modules and os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library() -> C.CDLL:
    """dlopen libalice_codec.so (built in-tree by ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP library is the product path and has no fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
    _preload_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    sig = {
        "alice_codec_wavelet1d_haar": (vp, []),
        "alice_codec_wavelet1d_cdf53": (vp, []),
        "alice_codec_wavelet1d_cdf97": (vp, []),
        "alice_codec_wavelet1d_destroy": (None, [vp]),
        "alice_codec_wavelet1d_forward": (None, [vp, _i32p, C.c_uint32]),
        "alice_codec_wavelet1d_inverse": (None, [vp, _i32p, C.c_uint32]),
        "alice_codec_encoder_create": (vp, [C.c_uint8]),
        "alice_codec_encoder_destroy": (None, [vp]),
        "alice_codec_encode": (vp, [vp, _u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "alice_codec_decode": (vp, [vp, _u32p]),
        "alice_codec_chunk_destroy": (None, [vp]),
        "alice_codec_chunk_to_bytes": (vp, [vp, _u32p]),
        "alice_codec_chunk_from_bytes": (vp, [_u8p, C.c_uint32]),
        "alice_codec_chunk_width": (C.c_uint32, [vp]),
        "alice_codec_chunk_height": (C.c_uint32, [vp]),
        "alice_codec_chunk_frames": (C.c_uint32, [vp]),
        "alice_codec_psnr": (C.c_double, [_u8p, _u8p, C.c_uint32]),
        "alice_codec_data_free": (None, [vp, C.c_uint32]),
        "alice_codec_string_free": (None, [vp]),
        "alice_codec_version": (vp, []),
        # extensions
        "alice_codec_last_error": (C.c_int, []),
        "alice_codec_last_error_message": (C.c_char_p, []),
        "alice_codec_device_count": (C.c_int, []),
        "alice_codec_set_device": (C.c_int, [C.c_int]),
        "alice_codec_trim": (None, []),
        "alice_codec_freq_table_from_histogram_n": (C.c_int, [_u32p, C.c_uint32, _u16p, _u16p]),
        "alice_codec_rans_encoder_new": (vp, []),
        "alice_codec_rans_encoder_destroy": (None, [vp]),
        "alice_codec_rans_encoder_encode": (C.c_int, [vp, C.c_uint16, C.c_uint16]),
        "alice_codec_rans_encoder_encode_symbols": (C.c_int, [vp, _u8p, C.c_uint64, _u16p, _u16p]),
        "alice_codec_rans_encoder_state": (C.c_uint32, [vp]),
        "alice_codec_rans_encoder_finish": (vp, [vp, _u64p]),
        "alice_codec_rans_decoder_new": (vp, [_u8p, C.c_uint64]),
        "alice_codec_rans_decoder_destroy": (None, [vp]),
        "alice_codec_rans_decoder_decode_n": (C.c_int, [vp, C.c_uint64, _u16p, _u16p, _u8p]),
        "alice_codec_rans_decoder_is_empty": (C.c_int, [vp]),
        "alice_codec_rans_decoder_state": (C.c_uint32, [vp]),
        "alice_codec_rans_decoder_position": (C.c_uint64, [vp]),
        "alice_codec_quantize_subband": (C.c_int, [C.c_int32, C.c_int32, _i32p, C.c_uint64, _i32p, C.c_uint64]),
        "alice_codec_dequantize_subband": (C.c_int, [C.c_int32, _i32p, C.c_uint64, _i32p, C.c_uint64]),
        "alice_codec_test_force_first_cap": (None, [C.c_uint64]),
        "alice_codec_test_last_decode_stats": (None, [_u32p]),
        "alice_codec_test_chain_occupancy": (C.c_int, [_u32p]),
        "alice_codec_test_decode_chains": (C.c_int, [C.c_uint32, C.POINTER(vp), _u64p, _u16p, _u16p, C.POINTER(vp), C.c_uint64, _u32p, vp]),
        "alice_codec_test_decode_chains_n": (C.c_int, [C.c_uint32, C.POINTER(vp), _u64p, _u16p, _u16p, C.POINTER(vp), _u64p, _u32p, vp]),
        "alice_codec_test_decode_chains_ex": (C.c_int, [C.c_uint32, C.POINTER(vp), _u64p, C.POINTER(vp), _u64p, _u32p, _u16p, _u16p, _u32p,
                                                        _u32p, _u32p, _u64p, _u32p, _u32p, vp]),
        "alice_codec_test_encode_chains": (C.c_int, [C.c_uint32, C.POINTER(vp), _u64p, _u32p, _u16p, _u16p, C.POINTER(vp), _u64p, _u32p, _u32p,
                                                     _u32p, vp]),
        "alice_codec_test_set_tuning": (None, [C.c_long]),
        "alice_codec_test_set_grid_cap": (None, [C.c_uint32]),
        "alice_codec_test_wide_symbols": (C.c_int, [_i32p, C.c_uint64, _u8p]),
        "alice_codec_test_transform_ms": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8,
                                                    C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_float), vp]),
        "alice_codec_encoder_create_ex": (vp, [C.c_uint8, C.c_uint8]),
        "alice_codec_encoder_quality": (C.c_uint8, [vp]),
        "alice_codec_encoder_wavelet": (C.c_uint8, [vp]),
        "alice_codec_chunk_wavelet": (C.c_uint8, [vp]),
        "alice_codec_chunk_compressed_size": (C.c_uint64, [vp]),
        "alice_codec_encode64": (vp, [vp, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]),
        "alice_codec_decode64": (vp, [vp, _u64p]),
        "alice_codec_chunk_to_bytes64": (vp, [vp, _u64p]),
        "alice_codec_chunk_from_bytes64": (vp, [_u8p, C.c_uint64]),
        "alice_codec_data_free64": (None, [vp, C.c_uint64]),
        "alice_codec_encode_many": (C.c_int, [vp, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
        "alice_codec_decode_many": (C.c_int, [C.POINTER(vp), C.c_uint32, _u8p, C.c_uint64]),
        "alice_codec_many_devices_plan": (C.c_int, [C.c_uint32, C.POINTER(C.c_int), C.c_uint32, C.POINTER(C.c_int)]),
        "alice_codec_encode_many_devices": (C.c_int, [vp, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                      C.POINTER(C.c_int), C.c_uint32, C.POINTER(vp)]),
        "alice_codec_decode_many_devices": (C.c_int, [C.POINTER(vp), C.c_uint32, C.POINTER(C.c_int), C.c_uint32, _u8p, C.c_uint64]),
        "alice_codec_batch_create": (vp, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8]),
        "alice_codec_batch_destroy": (None, [vp]),
        "alice_codec_batch_encode": (C.c_int, [vp, vp, vp]),
        "alice_codec_batch_encode_finish": (C.c_int, [vp, _u64p]),
        "alice_codec_batch_alc_ptr": (vp, [vp, C.c_uint32]),
        "alice_codec_batch_alc_stride": (C.c_uint64, [vp]),
        "alice_codec_batch_pack_alc": (C.c_int, [vp, _u64p, vp, C.c_uint64, vp]),
        "alice_codec_batch_decode": (C.c_int, [vp, vp, C.c_uint64, vp, vp]),
        "alice_codec_batch_encode_regions": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, _u32p, vp]),
        "alice_codec_batch_decode_regions": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, _u32p, vp]),
        "alice_codec_batch_decode_finish": (C.c_int, [vp]),
        "alice_codec_batch_stage_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "alice_codec_batch_symbols_ptr": (vp, [vp]),
        "alice_codec_batch_rgb_ptr": (vp, [vp, C.c_uint32]),
        "alice_codec_batch_padded_pixels": (C.c_uint64, [vp]),
        "alice_codec_batch_bytes_per_chunk": (C.c_uint64, [vp]),
        "alice_codec_batch_fixed_bytes": (C.c_uint64, [vp]),
        "alice_codec_wavelet2d_forward": (C.c_int, [C.c_uint8, _i32p, C.c_uint64, C.c_uint64]),
        "alice_codec_wavelet2d_inverse": (C.c_int, [C.c_uint8, _i32p, C.c_uint64, C.c_uint64]),
        "alice_codec_wavelet3d_forward": (C.c_int, [C.c_uint8, _i32p, C.c_uint64, C.c_uint64, C.c_uint64]),
        "alice_codec_wavelet3d_inverse": (C.c_int, [C.c_uint8, _i32p, C.c_uint64, C.c_uint64, C.c_uint64]),
        "alice_codec_quantize_buffer": (C.c_int, [C.c_int32, C.c_int32, _i32p, C.c_uint64, _i32p, C.c_uint64]),
        "alice_codec_dequantize_buffer": (C.c_int, [C.c_int32, _i32p, C.c_uint64, _i32p, C.c_uint64]),
        "alice_codec_fastquant_new": (vp, [C.c_int32]),
        "alice_codec_fastquant_with_dead_zone": (vp, [C.c_int32, C.c_int32]),
        "alice_codec_fastquant_destroy": (None, [vp]),
        "alice_codec_fastquant_step": (C.c_int32, [vp]),
        "alice_codec_fastquant_dead_zone": (C.c_int32, [vp]),
        "alice_codec_fastquant_quantize_buffer": (C.c_int, [vp, _i32p, C.c_uint64, _i32p, C.c_uint64]),
        "alice_codec_fastquant_dequantize_buffer": (C.c_int, [vp, _i32p, C.c_uint64, _i32p, C.c_uint64]),
        "alice_codec_to_symbols": (C.c_int, [_i32p, C.c_uint64, _u8p, C.c_uint64]),
        "alice_codec_from_symbols": (C.c_int, [_u8p, C.c_uint64, _i32p, C.c_uint64]),
        "alice_codec_build_histogram": (C.c_int, [_u8p, C.c_uint64, _u32p]),
        "alice_codec_freq_table_from_histogram": (C.c_int, [_u32p, _u16p, _u16p]),
        "alice_codec_rans_encode": (vp, [_u8p, C.c_uint64, _u16p, _u16p, _u64p]),
        "alice_codec_rans_decode": (C.c_int, [_u8p, C.c_uint64, _u16p, _u16p, C.c_uint64, _u8p]),
        "alice_codec_ssim": (C.c_double, [_u8p, C.c_uint64, _u8p, C.c_uint64, C.c_uint64, C.c_uint64]),
        "alice_codec_ms_ssim": (C.c_double, [_u8p, C.c_uint64, _u8p, C.c_uint64, C.c_uint64, C.c_uint64]),
        "alice_codec_rdo_target_bpp": (C.c_double, [C.c_uint8]),
        "alice_codec_subband_quant_strength": (C.c_uint8, [C.c_uint8]),
        "alice_codec_rdo_compute_quantizer": (C.c_int, [C.c_double, _i32p, C.c_uint64, C.c_uint8, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "alice_codec_rans_encode_interleaved": (vp, [_u8p, C.c_uint64, _u16p, _u16p, _u64p]),
        "alice_codec_rans_decode_interleaved": (C.c_int, [_u8p, C.c_uint64, _u16p, _u16p, C.c_uint64, _u8p]),
        "alice_codec_rgb_to_ycocg_r": (C.c_int, [_u8p, C.c_uint64, _i16p, _i16p, _i16p, C.c_uint64]),
        "alice_codec_ycocg_r_to_rgb": (C.c_int, [_i16p, _i16p, _i16p, C.c_uint64, _u8p, C.c_uint64]),
        "alice_codec_dev_forward_symbols": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8, vp, vp, vp]),
        "alice_codec_dev_inverse_symbols": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, _i32p, vp, vp]),
        "alice_codec_dev_wavelet3d_forward": (C.c_int, [C.c_uint8, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]),
        "alice_codec_dev_wavelet3d_inverse": (C.c_int, [C.c_uint8, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]),
        "alice_codec_dev_histogram": (C.c_int, [vp, C.c_uint64, vp, vp]),
        "alice_codec_rans_stream_bound": (C.c_uint64, [_u32p, C.c_uint64]),
        "alice_codec_dev_rans_encode": (C.c_int, [vp, C.c_uint64, _u32p, vp, C.c_uint64, _u64p, _u64p, vp]),
        "alice_codec_dev_rans_decode": (C.c_int, [vp, C.c_uint64, _u32p, vp, C.c_uint64, vp]),
        "alice_codec_segment_by_motion": (C.c_int, [_u8p, C.c_uint64, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint8,
                                                    C.c_uint32, C.c_uint32, _u8p, C.c_uint64, _u32p, _u32p]),
        "alice_codec_segment_by_chroma": (C.c_int, [_i16p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int16, _u8p, C.c_uint64,
                                                    _u32p, _u32p]),
        "alice_codec_rle_encode_mask": (vp, [_u8p, C.c_uint64, _u64p]),
        "alice_codec_extract_person_rgb": (C.c_int, [_u8p, C.c_uint64, C.c_uint32, _u32p, _u8p, C.c_uint64, _u8p, C.c_uint64,
                                                     _u64p]),
        "alice_codec_dev_segment_motion": (C.c_int, [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8,
                                                     C.c_uint32, C.c_uint32, vp, vp, vp]),
        "alice_codec_dev_segment_chroma_rgb": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int16, vp, vp, vp]),
        "alice_codec_rle_bound": (C.c_uint64, [C.c_uint64]),
        "alice_codec_dev_rle_encode_mask": (C.c_int, [vp, C.c_uint64, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_extract_person_rgb": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, vp, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_predict_sizes": (C.c_int, [C.c_uint8, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _u64p, _u64p, _u8p]),
        "alice_codec_encode_to_size": (vp, [C.c_uint8, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                            C.c_uint8, C.c_uint8, _u8p, _u8p]),
        "alice_codec_dev_predict_sizes": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, _u64p, _u64p,
                                                    _u8p, vp, vp]),
        "alice_codec_test_rate_log_table": (None, [_u32p, _u32p, _u32p]),
        "alice_codec_batch_predict_sizes": (C.c_int, [vp, vp, _u64p, _u64p, _u8p, vp]),
        "alice_codec_batch_set_qualities": (C.c_int, [vp, _u8p]),
        "alice_codec_batch_encode_to_budget": (C.c_int, [vp, vp, _u64p, C.c_uint8, C.c_uint8, _u8p, _u8p, vp]),
        "alice_codec_split_stream_bound": (C.c_uint64, [C.c_uint64, C.c_uint32]),
        "alice_codec_split_normalize": (C.c_int, [_u32p, _u16p]),
        "alice_codec_dev_split_encode": (C.c_int, [vp, C.c_uint64, _u32p, C.c_uint32, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_split_decode": (C.c_int, [vp, C.c_uint64, _u16p, C.c_uint32, vp, C.c_uint64, vp]),
        "alice_codec_encode_split": (vp, [vp, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u64p]),
        "alice_codec_decode_split": (vp, [_u8p, C.c_uint64, _u64p]),
        "alice_codec_split_info": (C.c_int, [_u8p, C.c_uint64, vp]),
        "alice_codec_dev_encode_split": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8, _u8p,
                                                   C.c_uint32, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_decode_split": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, vp, vp]),
        "alice_codec_wide_stream_bound": (C.c_uint64, [C.c_uint64, C.c_uint32]),
        "alice_codec_dev_wide_encode": (C.c_int, [vp, C.c_uint64, _u32p, C.c_uint32, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_wide_decode": (C.c_int, [vp, C.c_uint64, _u16p, C.c_uint32, vp, C.c_uint64, vp]),
        "alice_codec_encode_wide": (vp, [vp, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u64p]),
        "alice_codec_decode_wide": (vp, [_u8p, C.c_uint64, _u64p]),
        "alice_codec_wide_info": (C.c_int, [_u8p, C.c_uint64, vp]),
        "alice_codec_dev_encode_wide": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8, _u8p,
                                                  C.c_uint32, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_decode_wide": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, vp, vp]),
        "alice_codec_dev_forward_symbols_wide": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8, vp, vp, vp]),
        "alice_codec_predict_split_sizes": (C.c_int, [C.c_uint8, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                      _u64p, _u64p]),
        "alice_codec_dev_predict_split_sizes": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint32,
                                                          _u64p, _u64p, vp]),
        "alice_codec_encode_split_to_size": (vp, [C.c_uint8, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.c_uint64, C.c_uint8, C.c_uint8, _u8p, _u8p, _u64p]),
        "alice_codec_dev_encode_split_regions": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                           C.c_uint32, C.c_uint8, C.c_uint8, _u8p, C.c_uint32, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_decode_split_regions": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, vp, C.c_uint32, C.c_uint32, _u32p, vp]),
        "alice_codec_dev_encode_split_to_budget": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                             C.c_uint32, C.c_uint8, C.c_uint32, _u64p, C.c_uint8, C.c_uint8, _u8p, _u8p,
                                                             vp, C.c_uint64, _u64p, vp]),
        "alice_codec_encode_reversible": (vp, [vp, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u64p]),
        "alice_codec_decode_reversible": (vp, [_u8p, C.c_uint64, _u64p]),
        "alice_codec_reversible_info": (C.c_int, [_u8p, C.c_uint64, vp]),
        "alice_codec_dev_encode_reversible": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8, _u8p,
                                                        C.c_uint32, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_decode_reversible": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, vp, vp]),
        "alice_codec_dev_encode_reversible_regions": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                                C.c_uint32, C.c_uint8, C.c_uint8, _u8p, C.c_uint32, vp, C.c_uint64,
                                                                _u64p, vp]),
        "alice_codec_dev_decode_reversible_regions": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, vp, C.c_uint32, C.c_uint32, _u32p,
                                                                vp]),
        "alice_codec_predict_wide_sizes": (C.c_int, [C.c_uint8, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                     _u64p, _u64p]),
        "alice_codec_dev_predict_wide_sizes": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint32,
                                                         _u64p, _u64p, vp, vp]),
        "alice_codec_encode_wide_to_size": (vp, [C.c_uint8, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                 C.c_uint64, C.c_uint8, C.c_uint8, _u8p, _u8p, _u64p]),
        "alice_codec_dev_encode_wide_regions": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                          C.c_uint32, C.c_uint8, C.c_uint8, _u8p, C.c_uint32, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_decode_wide_regions": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, vp, C.c_uint32, C.c_uint32, _u32p, vp]),
        "alice_codec_dev_encode_wide_to_budget": (C.c_int, [vp, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                            C.c_uint32, C.c_uint8, C.c_uint32, _u64p, C.c_uint8, C.c_uint8, _u8p, _u8p,
                                                            vp, C.c_uint64, _u64p, vp]),
        "alice_codec_test_last_split_trials": (C.c_uint32, [_u32p, C.c_uint32]),
        "alice_codec_dev_rgb_sse": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                              C.c_uint64, vp, vp]),
        "alice_codec_dev_trial_sse": (C.c_int, [C.c_uint8, vp, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint8, C.c_uint8, _u8p, _u64p, vp, vp]),
        "alice_codec_psnr_from_sse": (C.c_double, [C.c_uint64, C.c_uint64]),
        "alice_codec_dev_encode_to_psnr": (C.c_int, [C.c_uint8, vp, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                     C.c_uint32, C.c_uint8, C.c_uint32, C.c_double, C.c_uint8, C.c_uint8, _u8p, _u8p,
                                                     C.POINTER(C.c_double), vp, C.c_uint64, _u64p, vp]),
        "alice_codec_encode_to_psnr": (vp, [C.c_uint8, C.c_uint8, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_double, C.c_uint8, C.c_uint8, _u8p, _u8p, C.POINTER(C.c_double), _u64p]),
        "alice_codec_test_last_quality_trials": (C.c_uint32, [_u32p, C.c_uint32]),
        "alice_codec_test_inverse_scratch_bytes": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
        "alice_codec_test_group_scratch_bytes": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int]),
        "alice_codec_test_set_group_chunks": (None, [C.c_uint32]),
        "alice_codec_test_group_chunks": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
        "alice_codec_test_sq_diff_sum": (C.c_int, [vp, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_test_inverse_variant": (C.c_int, [C.c_uint8, _i32p, C.c_int]),
        "alice_codec_frames_window": (C.c_int, [C.c_uint8, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p]),
        "alice_codec_decode_frames": (vp, [_u8p, C.c_uint64, C.c_uint32, C.c_uint32, _u64p]),
        "alice_codec_dev_decode_frames": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp]),
        "alice_codec_test_last_frames_stats": (None, [_u64p]),
        "alice_codec_preview_dims": (C.c_int, [C.c_uint32, C.c_uint32, _u32p, _u32p]),
        "alice_codec_decode_preview": (vp, [_u8p, C.c_uint64, C.c_uint32, C.c_uint32, _u64p]),
        "alice_codec_dev_decode_preview": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp]),
        "alice_codec_test_last_preview_stats": (None, [_u64p]),
        "alice_codec_decode_previews": (vp, [C.POINTER(PreviewItem), C.c_uint32, _u64p, _u32p]),
        "alice_codec_dev_decode_previews": (C.c_int, [C.POINTER(PreviewItem), C.c_uint32, _u32p, vp]),
        "alice_codec_test_last_previews_stats": (None, [_u64p]),
        "alice_codec_rect_window": (C.c_int, [C.c_uint8] + [C.c_uint32] * 6 + [_u32p] * 4),
        "alice_codec_decode_rect": (vp, [_u8p, C.c_uint64] + [C.c_uint32] * 6 + [_u64p]),
        "alice_codec_dev_decode_rect": (C.c_int, [vp, C.c_uint64] + [C.c_uint32] * 6 + [vp, C.c_uint64, C.c_uint64, vp]),
        "alice_codec_test_last_rect_stats": (None, [_u64p]),
        "alice_codec_decode_rects": (vp, [C.POINTER(RectItem), C.c_uint32, _u64p, _u32p]),
        "alice_codec_dev_decode_rects": (C.c_int, [C.POINTER(RectItem), C.c_uint32, _u32p, vp]),
        "alice_codec_test_last_rects_stats": (None, [_u64p]),
        "alice_codec_test_rects_outputs_disjoint": (C.c_int, [C.POINTER(RectItem), C.c_uint32, _u32p]),
        "alice_codec_transcode": (vp, [_u8p, C.c_uint64, C.c_uint8, C.c_uint32, C.c_uint8, _u64p]),
        "alice_codec_transcode_to_size": (vp, [_u8p, C.c_uint64, C.c_uint32, C.c_uint8, C.c_uint64, C.c_uint8, C.c_uint8, _u8p, _u8p, _u64p]),
        "alice_codec_predict_transcode_sizes": (C.c_int, [_u8p, C.c_uint64, C.c_uint32, _u64p, _u64p]),
        "alice_codec_dev_transcode": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, C.c_uint8, _u8p, C.c_uint32, C.c_uint8, vp, C.c_uint64,
                                                _u64p, vp]),
        "alice_codec_dev_transcode_to_budget": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, C.c_uint32, C.c_uint8, _u64p, C.c_uint8, C.c_uint8,
                                                          _u8p, _u8p, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_requant_symbols": (C.c_int, [vp, vp, C.c_uint64, C.c_int, C.c_int32, C.c_int32, vp, vp]),
        "alice_codec_test_symbol_bins": (C.c_int, [vp, C.c_uint64, C.c_int, C.c_int32, vp, vp, vp]),
        "alice_codec_banded_stream_bound": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint8]),
        "alice_codec_banded_info": (C.c_int, [_u8p, C.c_uint64, vp]),
        "alice_codec_encode_banded": (vp, [vp, _u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, _u64p]),
        "alice_codec_decode_banded": (vp, [_u8p, C.c_uint64, _u64p]),
        "alice_codec_dev_encode_banded": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_uint8, _u8p,
                                                    C.c_uint32, C.c_uint8, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_decode_banded": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, vp, vp]),
        "alice_codec_to_banded": (vp, [_u8p, C.c_uint64, C.c_uint32, _u64p]),
        "alice_codec_from_banded": (vp, [_u8p, C.c_uint64, C.c_uint32, _u64p]),
        "alice_codec_dev_to_banded": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, C.c_uint32, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_from_banded": (C.c_int, [vp, C.c_uint64, _u64p, C.c_uint32, C.c_uint32, vp, C.c_uint64, _u64p, vp]),
        "alice_codec_dev_band_histograms": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, vp]),
        "alice_codec_decode_banded_frames": (vp, [_u8p, C.c_uint64, C.c_uint32, C.c_uint32, _u64p]),
        "alice_codec_dev_decode_banded_frames": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp]),
        "alice_codec_decode_banded_preview": (vp, [_u8p, C.c_uint64, C.c_uint32, C.c_uint32, _u64p]),
        "alice_codec_dev_decode_banded_preview": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp]),
        "alice_codec_test_last_banded_frames_stats": (None, [_u64p]),
        "alice_codec_test_last_banded_preview_stats": (None, [_u64p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTED_SYMBOLS_PART1 = [
    "alice_codec_wavelet1d_haar", "alice_codec_wavelet1d_cdf53", "alice_codec_wavelet1d_cdf97",
    "alice_codec_wavelet1d_destroy", "alice_codec_wavelet1d_forward", "alice_codec_wavelet1d_inverse",
    "alice_codec_encoder_create", "alice_codec_encoder_destroy", "alice_codec_encode", "alice_codec_decode",
    "alice_codec_chunk_destroy", "alice_codec_chunk_to_bytes", "alice_codec_chunk_from_bytes",
    "alice_codec_chunk_width", "alice_codec_chunk_height", "alice_codec_chunk_frames", "alice_codec_psnr",
    "alice_codec_data_free", "alice_codec_string_free", "alice_codec_version",
]


def _raise_last(default_code: int = 10):
    lib = load_library()
    code = lib.alice_codec_last_error() or default_code
    msg = lib.alice_codec_last_error_message()
    raise CodecError(code, msg.decode("utf-8", "replace") if msg else "")


def _check(rc: int):
    if rc != 0:
        _raise_last(rc)


def _copy_out(ptr, n: int) -> np.ndarray:
    """Copies n bytes at a C pointer into a fresh array.  (ctypes.string_at takes its size as a C int on this
    Python, which silently truncates buffers of 2 GiB and more.)"""
    if n == 0:
        return np.zeros(0, np.uint8)
    addr = C.cast(ptr, C.c_void_p).value
    return np.frombuffer((C.c_uint8 * n).from_address(addr), dtype=np.uint8).copy()


def _adopt(ptr, n: int, free_fn) -> np.ndarray:
    """A uint8 array over n bytes the library allocated, without copying them: the array's base owns the C buffer and
    hands it to free_fn(ptr, n) when the last reference goes (FrameDecoder.decode: 398 MB per 1080p x 64 chunk)."""
    if n == 0:
        free_fn(ptr, n)
        return np.zeros(0, np.uint8)
    addr = C.cast(ptr, C.c_void_p).value
    buf = (C.c_uint8 * n).from_address(addr)
    weakref.finalize(buf, free_fn, addr, n)
    return np.frombuffer(buf, dtype=np.uint8)


def _as_u8(a) -> np.ndarray:
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(a, dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


def _p(a: np.ndarray, t):
    return a.ctypes.data_as(t)


def device_count() -> int:
    return load_library().alice_codec_device_count()


def set_device(i: int) -> None:
    _check(load_library().alice_codec_set_device(i))


def version() -> str:
    lib = load_library()
    p = lib.alice_codec_version()
    try:
        return C.string_at(p).decode()
    finally:
        lib.alice_codec_string_free(p)


# ---------------------------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------------------------

class EncodedChunk:
    """reference src/pipeline.rs:172-313 (handle owned by the library)."""

    def __init__(self, handle: int):
        if not handle:
            raise ValueError("null chunk handle")
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.alice_codec_chunk_destroy(h)

    @property
    def width(self) -> int:
        return load_library().alice_codec_chunk_width(self._h)

    @property
    def height(self) -> int:
        return load_library().alice_codec_chunk_height(self._h)

    @property
    def frames(self) -> int:
        return load_library().alice_codec_chunk_frames(self._h)

    @property
    def wavelet_type(self) -> WaveletType:
        return WaveletType(load_library().alice_codec_chunk_wavelet(self._h))

    def compressed_size(self) -> int:
        return load_library().alice_codec_chunk_compressed_size(self._h)

    def to_bytes(self) -> bytes:
        lib = load_library()
        n = C.c_uint64()
        p = lib.alice_codec_chunk_to_bytes64(self._h, C.byref(n))
        if not p:
            _raise_last()
        try:
            return _copy_out(p, n.value).tobytes()
        finally:
            lib.alice_codec_data_free64(p, n.value)

    @staticmethod
    def from_bytes(data) -> "EncodedChunk":
        lib = load_library()
        d = _as_u8(data)
        h = lib.alice_codec_chunk_from_bytes64(_p(d, _u8p) if d.size else C.cast(C.c_char_p(b""), _u8p), d.size)
        if not h:
            _raise_last(4)
        return EncodedChunk(h)


class FrameEncoder:
    """reference src/pipeline.rs:335-507.  ``FrameEncoder(q)`` = ``new``; ``with_wavelet`` as in the reference."""

    def __init__(self, quality: int, wavelet_type: WaveletType = WaveletType.Cdf53):
        lib = load_library()
        # the reference takes a u8 (src/pipeline.rs:347): an out-of-range value is a caller error there (clap / PyO3
        # refuse it), never a silent wrap
        if not 0 <= int(quality) <= 255:
            raise ValueError(f"quality must fit a u8 (0..255), got {quality}")
        self.quality = int(quality)
        self.wavelet_type = WaveletType(wavelet_type)
        self._h = lib.alice_codec_encoder_create_ex(self.quality, int(self.wavelet_type))
        if not self._h:
            _raise_last()

    @classmethod
    def with_wavelet(cls, quality: int, wavelet_type: WaveletType) -> "FrameEncoder":
        return cls(quality, wavelet_type)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.alice_codec_encoder_destroy(h)

    def encode(self, rgb_frames, width: int, height: int, frames: int) -> EncodedChunk:
        lib = load_library()
        r = _as_u8(rgb_frames)
        for v in (width, height, frames):
            if not 0 <= v <= 0xFFFFFFFF:
                raise CodecError(3, "dimension out of u32 range")
        ptr = _p(r, _u8p) if r.size else C.cast(C.c_char_p(b""), _u8p)
        h = lib.alice_codec_encode64(self._h, ptr, r.size, width, height, frames)
        if not h:
            _raise_last()
        return EncodedChunk(h)


# ---------------------------------------------------------------------------------------------
# rate control: sizes at every quality before encoding, encodes to a byte budget
# ---------------------------------------------------------------------------------------------

from .rate_control import RateControlConfig, RateController, estimate_quality, budget_bytes_per_chunk  # noqa: E402

RATE_BOUNDED, RATE_UNBOUNDED, RATE_DIVERGES = 0, 1, 2


class SizePrediction:
    """Predicted .alc lengths of a chunk at the 101 qualities: ``lo[q] <= len(chunk.to_bytes()) <= hi[q]`` wherever
    ``status[q] == RATE_BOUNDED`` (otherwise lo = 0 and hi = 2^64 - 1).  Arrays of 101 entries, or (n_chunks, 101)."""

    def __init__(self, lo: np.ndarray, hi: np.ndarray, status: np.ndarray):
        self.lo, self.hi, self.status = lo, hi, status

    def choose(self, budget: int, min_quality: int = 10, max_quality: int = 95) -> tuple:
        """The budget rule of encode_to_size for one chunk: (quality, fits)."""
        lo_q, hi_q = min(int(min_quality), 100), min(int(max_quality), 100)
        for q in range(hi_q, lo_q - 1, -1):
            if self.status[q] == RATE_BOUNDED and int(self.hi[q]) <= budget:
                return q, True
        return lo_q, False


def _check_budget_args(budgets, min_quality, max_quality):
    for q in (min_quality, max_quality):
        if not 0 <= int(q) <= 255:
            raise ValueError(f"quality must fit a u8 (0..255), got {q}")
    for b in budgets:
        if not 0 <= int(b) < (1 << 64):
            raise ValueError(f"a byte budget must fit a u64 (0 .. 2^64 - 1), got {b}")


def _dims_u32(*vals):
    for v in vals:
        if not 0 <= v <= 0xFFFFFFFF:
            raise CodecError(3, "dimension out of u32 range")


def predict_sizes(rgb_frames, width: int, height: int, frames: int,
                  wavelet_type: WaveletType = WaveletType.Cdf53) -> SizePrediction:
    """The size bracket of FrameEncoder.with_wavelet(q, wavelet_type).encode(...) at every quality q, from one forward
    transform on the GPU (no entropy coding)."""
    lib = load_library()
    r = _as_u8(rgb_frames)
    _dims_u32(width, height, frames)
    lo = np.zeros(101, np.uint64); hi = np.zeros(101, np.uint64); st = np.zeros(101, np.uint8)
    ptr = _p(r, _u8p) if r.size else C.cast(C.c_char_p(b""), _u8p)
    _check(lib.alice_codec_predict_sizes(int(wavelet_type), ptr, r.size, width, height, frames,
                                         _p(lo, _u64p), _p(hi, _u64p), _p(st, _u8p)))
    return SizePrediction(lo, hi, st)


def predict_sizes_device(d_rgb_ptr: int, width: int, height: int, frames: int, n_chunks: int,
                         wavelet_type: WaveletType = WaveletType.Cdf53, d_step_hist_ptr: int | None = None,
                         stream: int = 0) -> SizePrediction:
    """n_chunks packed chunks at a device pointer: arrays of shape (n_chunks, 101).  d_step_hist_ptr (optional, device,
    n_chunks * 64 * 3 * 256 u32) receives the symbol histograms at every quantiser step."""
    lib = load_library()
    _dims_u32(width, height, frames, n_chunks)
    lo = np.zeros((max(n_chunks, 1), 101), np.uint64); hi = np.zeros_like(lo); st = np.zeros(lo.shape, np.uint8)
    _check(lib.alice_codec_dev_predict_sizes(d_rgb_ptr, width, height, frames, n_chunks, int(wavelet_type), _p(lo, _u64p),
                                             _p(hi, _u64p), _p(st, _u8p), d_step_hist_ptr, stream))
    return SizePrediction(lo[:n_chunks], hi[:n_chunks], st[:n_chunks])


def encode_to_size(rgb_frames, width: int, height: int, frames: int, max_bytes: int,
                   wavelet_type: WaveletType = WaveletType.Cdf53, min_quality: int = 10, max_quality: int = 95) -> tuple:
    """Encodes one chunk once, at the highest quality in [min_quality, max_quality] whose predicted .alc length is
    guaranteed to fit max_bytes.  Returns (EncodedChunk, quality, fits); fits is False when not even min_quality is
    guaranteed to fit (the chunk is then encoded at min_quality)."""
    lib = load_library()
    r = _as_u8(rgb_frames)
    _dims_u32(width, height, frames)
    _check_budget_args([max_bytes], min_quality, max_quality)
    chosen = C.c_uint8(0); fits = C.c_uint8(0)
    ptr = _p(r, _u8p) if r.size else C.cast(C.c_char_p(b""), _u8p)
    h = lib.alice_codec_encode_to_size(int(wavelet_type), ptr, r.size, width, height, frames, int(max_bytes),
                                       int(min_quality), int(max_quality), C.byref(chosen), C.byref(fits))
    if not h:
        _raise_last()
    return EncodedChunk(h), int(chosen.value), bool(fits.value)


def plan_devices(n_chunks: int, devices) -> list:
    """Which device each chunk of a multi-device call runs on: chunk k -> devices[k mod len(devices)] (no GPU touched)."""
    devs = (C.c_int * len(devices))(*[int(x) for x in devices])
    out = (C.c_int * max(n_chunks, 1))()
    _check(load_library().alice_codec_many_devices_plan(n_chunks, devs, len(devices), out))
    return list(out)[:n_chunks]


def encode_many(encoder: "FrameEncoder", rgb_chunks, width: int, height: int, frames: int, devices=None) -> list:
    """n equal-shaped chunks (array of shape [n, frames*height*width*3] or a flat buffer) in one call: all their
    entropy chains run side by side.  Returns n EncodedChunk, identical to n FrameEncoder.encode calls.
    devices: a list of GPU indices -- chunk k runs on devices[k mod len(devices)], one host thread per entry."""
    lib = load_library()
    r = _as_u8(rgb_chunks)
    per = width * height * frames * 3
    if per == 0 or r.size % per:
        raise CodecError(1, "buffer is not a whole number of chunks")
    n = r.size // per
    handles = (C.c_void_p * n)()
    if devices is None:
        _check(lib.alice_codec_encode_many(encoder._h, _p(r, _u8p), r.size, width, height, frames, n, handles))
    else:
        devs = (C.c_int * len(devices))(*[int(x) for x in devices])
        _check(lib.alice_codec_encode_many_devices(encoder._h, _p(r, _u8p), r.size, width, height, frames, n, devs, len(devices), handles))
    return [EncodedChunk(h) for h in handles]


def decode_many(chunks, devices=None) -> np.ndarray:
    """n equal-shaped chunks -> uint8 array [n, frames*height*width*3]; devices as in encode_many"""
    lib = load_library()
    n = len(chunks)
    if n == 0:
        return np.zeros((0, 0), np.uint8)
    per = chunks[0].width * chunks[0].height * chunks[0].frames * 3
    out = np.zeros((n, per), np.uint8)
    handles = (C.c_void_p * n)(*[c._h for c in chunks])
    z = C.cast(C.c_char_p(b""), _u8p)
    if devices is None:
        _check(lib.alice_codec_decode_many(handles, n, _p(out, _u8p) if out.size else z, out.size))
    else:
        devs = (C.c_int * len(devices))(*[int(x) for x in devices])
        _check(lib.alice_codec_decode_many_devices(handles, n, devs, len(devices), _p(out, _u8p) if out.size else z, out.size))
    return out


class FrameDecoder:
    """reference src/pipeline.rs:519-631."""

    def decode(self, chunk: EncodedChunk) -> np.ndarray:
        lib = load_library()
        n = C.c_uint64()
        p = lib.alice_codec_decode64(chunk._h, C.byref(n))
        if not p:
            _raise_last()
        return _adopt(p, n.value, lib.alice_codec_data_free64)


def psnr(a, b) -> float:
    """metrics::psnr via the C ABI (src/ffi.rs:270-278): -1.0 on length mismatch."""
    a, b = _as_u8(a), _as_u8(b)
    if a.size != b.size:
        return -1.0
    z = C.cast(C.c_char_p(b""), _u8p)
    return load_library().alice_codec_psnr(_p(a, _u8p) if a.size else z, _p(b, _u8p) if b.size else z, a.size)


# ---------------------------------------------------------------------------------------------
# wavelets
# ---------------------------------------------------------------------------------------------

def _ssim(a, b, width: int, height: int, fn) -> float:
    a = _as_u8(a); b = _as_u8(b)
    z = C.cast(C.c_char_p(b""), _u8p)
    v = fn(_p(a, _u8p) if a.size else z, a.size, _p(b, _u8p) if b.size else z, b.size, width, height)
    if v == -1.0 and load_library().alice_codec_last_error() != 0:
        _raise_last(1)
    return v


def ssim(a, b, width: int, height: int) -> float:
    """reference src/ssim.rs:63-115"""
    return _ssim(a, b, width, height, load_library().alice_codec_ssim)


def ms_ssim(a, b, width: int, height: int) -> float:
    """reference src/ssim.rs:125-176"""
    return _ssim(a, b, width, height, load_library().alice_codec_ms_ssim)


class Wavelet1D:
    """reference src/wavelet.rs:47-249 through the 6 drop-in FFI functions (src/ffi.rs:16-86)."""

    def __init__(self, kind: WaveletType):
        lib = load_library()
        self.kind = WaveletType(kind)
        ctor = {WaveletType.Cdf53: lib.alice_codec_wavelet1d_cdf53, WaveletType.Cdf97: lib.alice_codec_wavelet1d_cdf97,
                WaveletType.Haar: lib.alice_codec_wavelet1d_haar}[self.kind]
        self._h = ctor()

    @classmethod
    def cdf97(cls): return cls(WaveletType.Cdf97)

    @classmethod
    def cdf53(cls): return cls(WaveletType.Cdf53)

    @classmethod
    def haar(cls): return cls(WaveletType.Haar)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.alice_codec_wavelet1d_destroy(h)

    def _run(self, signal, fn) -> np.ndarray:
        s = np.array(signal, dtype=np.int32).reshape(-1).copy()
        if s.size:
            fn(self._h, _p(s, _i32p), s.size)
            if load_library().alice_codec_last_error():
                _raise_last()
        return s

    def forward(self, signal) -> np.ndarray:
        return self._run(signal, load_library().alice_codec_wavelet1d_forward)

    def inverse(self, signal) -> np.ndarray:
        return self._run(signal, load_library().alice_codec_wavelet1d_inverse)


class Wavelet2D:
    """reference src/wavelet.rs:265-341."""

    def __init__(self, kind: WaveletType = WaveletType.Cdf53):
        self.kind = WaveletType(kind)

    @classmethod
    def cdf97(cls): return cls(WaveletType.Cdf97)

    @classmethod
    def cdf53(cls): return cls(WaveletType.Cdf53)

    def forward(self, image, width: int, height: int) -> np.ndarray:
        s = np.array(image, dtype=np.int32).reshape(-1).copy()
        assert s.size == width * height
        if s.size:
            _check(load_library().alice_codec_wavelet2d_forward(int(self.kind), _p(s, _i32p), width, height))
        return s

    def inverse(self, image, width: int, height: int) -> np.ndarray:
        s = np.array(image, dtype=np.int32).reshape(-1).copy()
        assert s.size == width * height
        if s.size:
            _check(load_library().alice_codec_wavelet2d_inverse(int(self.kind), _p(s, _i32p), width, height))
        return s


class Wavelet3D:
    """reference src/wavelet.rs:358-485."""

    def __init__(self, kind: WaveletType = WaveletType.Cdf53):
        self.kind = WaveletType(kind)

    @classmethod
    def cdf97(cls): return cls(WaveletType.Cdf97)

    @classmethod
    def cdf53(cls): return cls(WaveletType.Cdf53)

    def forward(self, volume, width: int, height: int, depth: int) -> np.ndarray:
        s = np.array(volume, dtype=np.int32).reshape(-1).copy()
        assert s.size == width * height * depth
        if s.size:
            _check(load_library().alice_codec_wavelet3d_forward(int(self.kind), _p(s, _i32p), width, height, depth))
        return s

    def inverse(self, volume, width: int, height: int, depth: int) -> np.ndarray:
        s = np.array(volume, dtype=np.int32).reshape(-1).copy()
        assert s.size == width * height * depth
        if s.size:
            _check(load_library().alice_codec_wavelet3d_inverse(int(self.kind), _p(s, _i32p), width, height, depth))
        return s


# ---------------------------------------------------------------------------------------------
# quantisers, symbols, histogram
# ---------------------------------------------------------------------------------------------

class Quantizer:
    """reference src/quant.rs:57-153."""

    def __init__(self, step: int, dead_zone: int | None = None):
        self.step = int(step)
        self.dead_zone = int(step if dead_zone is None else dead_zone)

    @classmethod
    def with_dead_zone(cls, step: int, dead_zone: int): return cls(step, dead_zone)

    def quantize_buffer(self, values, out_len: int | None = None) -> np.ndarray:
        v = np.ascontiguousarray(values, np.int32).reshape(-1)
        out = np.zeros(v.size if out_len is None else out_len, np.int32)
        _check(load_library().alice_codec_quantize_buffer(self.step, self.dead_zone, _p(v, _i32p), v.size, _p(out, _i32p), out.size))
        return out

    def dequantize_buffer(self, values, out_len: int | None = None) -> np.ndarray:
        v = np.ascontiguousarray(values, np.int32).reshape(-1)
        out = np.zeros(v.size if out_len is None else out_len, np.int32)
        _check(load_library().alice_codec_dequantize_buffer(self.step, _p(v, _i32p), v.size, _p(out, _i32p), out.size))
        return out

    def quantize(self, value: int) -> int:
        return int(self.quantize_buffer([value])[0])

    def dequantize(self, q: int) -> int:
        return int(self.dequantize_buffer([q])[0])


def quantize_subband(coeffs, quantizer: Quantizer, out_len: int | None = None) -> np.ndarray:
    """reference src/quant.rs:518-524"""
    v = np.ascontiguousarray(coeffs, np.int32).reshape(-1)
    out = np.zeros(v.size if out_len is None else out_len, np.int32)
    _check(load_library().alice_codec_quantize_subband(quantizer.step, quantizer.dead_zone, _p(v, _i32p), v.size, _p(out, _i32p), out.size))
    return out


def dequantize_subband(coeffs, quantizer: Quantizer, out_len: int | None = None) -> np.ndarray:
    """reference src/quant.rs:531-537"""
    v = np.ascontiguousarray(coeffs, np.int32).reshape(-1)
    out = np.zeros(v.size if out_len is None else out_len, np.int32)
    _check(load_library().alice_codec_dequantize_subband(quantizer.step, _p(v, _i32p), v.size, _p(out, _i32p), out.size))
    return out


class SubBand3D(enum.IntEnum):  # reference src/lib.rs:115-158
    LLL = 0
    LLH = 1
    LHL = 2
    LHH = 3
    HLL = 4
    HLH = 5
    HHL = 6
    HHH = 7

    def is_temporal_high(self) -> bool: return self in (SubBand3D.LLH, SubBand3D.LHH, SubBand3D.HLH, SubBand3D.HHH)

    def is_dc(self) -> bool: return self is SubBand3D.LLL

    def quant_strength(self) -> int: return int(load_library().alice_codec_subband_quant_strength(int(self)))


class AnalyticalRDO:
    """reference src/quant.rs:377-505: closed-form step per sub-band from the coefficient variance."""

    def __init__(self, target_bpp: float):            # AnalyticalRDO::new
        self._target_bpp, self._quality = float(target_bpp), 75

    @classmethod
    def with_quality(cls, quality: int) -> "AnalyticalRDO":
        q = min(int(quality), 100)
        r = cls(load_library().alice_codec_rdo_target_bpp(q))
        r._quality = q
        return r

    def quality(self) -> int: return self._quality

    def target_bpp(self) -> float: return self._target_bpp

    def compute_quantizer(self, coeffs, subband: SubBand3D) -> Quantizer:
        c = np.ascontiguousarray(coeffs, dtype=np.int32).reshape(-1)
        st, dz = C.c_int32(), C.c_int32()
        z = C.cast(C.c_char_p(b"\0\0\0\0"), _i32p)
        _check(load_library().alice_codec_rdo_compute_quantizer(self._target_bpp, _p(c, _i32p) if c.size else z, c.size, int(subband),
                                                                C.byref(st), C.byref(dz)))
        return Quantizer.with_dead_zone(st.value, dz.value)

    def compute_all_quantizers(self, subbands) -> list:
        return [self.compute_quantizer(c, SubBand3D(i)) for i, c in enumerate(subbands)]


class FastQuantizer:
    """reference src/quant.rs:171-359."""

    def __init__(self, step: int, dead_zone: int | None = None):
        lib = load_library()
        self._h = lib.alice_codec_fastquant_new(step) if dead_zone is None else lib.alice_codec_fastquant_with_dead_zone(step, dead_zone)
        if not self._h:
            _raise_last(5)

    @classmethod
    def with_dead_zone(cls, step: int, dead_zone: int): return cls(step, dead_zone)

    @classmethod
    def from_quantizer(cls, q: Quantizer): return cls(q.step, q.dead_zone)  # From<Quantizer>, :355-359

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.alice_codec_fastquant_destroy(h)

    def step(self) -> int: return load_library().alice_codec_fastquant_step(self._h)

    def dead_zone(self) -> int: return load_library().alice_codec_fastquant_dead_zone(self._h)

    def quantize_buffer(self, values, out_len: int | None = None) -> np.ndarray:
        v = np.ascontiguousarray(values, np.int32).reshape(-1)
        out = np.zeros(v.size if out_len is None else out_len, np.int32)
        _check(load_library().alice_codec_fastquant_quantize_buffer(self._h, _p(v, _i32p), v.size, _p(out, _i32p), out.size))
        return out

    quantize_buffer_simd = quantize_buffer  # :322-332 (same results by contract)

    def dequantize_buffer(self, values, out_len: int | None = None) -> np.ndarray:
        v = np.ascontiguousarray(values, np.int32).reshape(-1)
        out = np.zeros(v.size if out_len is None else out_len, np.int32)
        _check(load_library().alice_codec_fastquant_dequantize_buffer(self._h, _p(v, _i32p), v.size, _p(out, _i32p), out.size))
        return out

    def quantize(self, value: int) -> int: return int(self.quantize_buffer([value])[0])

    def dequantize(self, q: int) -> int: return int(self.dequantize_buffer([q])[0])


def to_symbols(coeffs, out_len: int | None = None) -> np.ndarray:
    v = np.ascontiguousarray(coeffs, np.int32).reshape(-1)
    out = np.zeros(v.size if out_len is None else out_len, np.uint8)
    _check(load_library().alice_codec_to_symbols(_p(v, _i32p), v.size, _p(out, _u8p), out.size))
    return out


def from_symbols(symbols, out_len: int | None = None) -> np.ndarray:
    s = _as_u8(symbols)
    out = np.zeros(s.size if out_len is None else out_len, np.int32)
    _check(load_library().alice_codec_from_symbols(_p(s, _u8p), s.size, _p(out, _i32p), out.size))
    return out


def build_histogram(symbols) -> np.ndarray:
    s = _as_u8(symbols)
    out = np.zeros(256, np.uint32)
    z = C.cast(C.c_char_p(b""), _u8p)
    _check(load_library().alice_codec_build_histogram(_p(s, _u8p) if s.size else z, s.size, _p(out, _u32p)))
    return out


# ---------------------------------------------------------------------------------------------
# rANS
# ---------------------------------------------------------------------------------------------

class FrequencyTable:
    """reference src/rans.rs:85-219.  n symbols, 1 <= n <= 256 (the coders address symbols as u8); the arrays always
    hold 256 entries, those from n on are (0, 0)."""

    def __init__(self, cum_freq: np.ndarray, freq: np.ndarray, n_symbols: int = 256):
        self.cum_freq = np.ascontiguousarray(cum_freq, np.uint16)
        self.freq = np.ascontiguousarray(freq, np.uint16)
        self._n = int(n_symbols)

    @classmethod
    def from_histogram(cls, histogram) -> "FrequencyTable":
        h = np.ascontiguousarray(histogram, np.uint32).reshape(-1)
        cum = np.zeros(256, np.uint16); fr = np.zeros(256, np.uint16)
        z = C.cast(C.c_char_p(b""), _u32p)
        _check(load_library().alice_codec_freq_table_from_histogram_n(_p(h, _u32p) if h.size else z, h.size, _p(cum, _u16p), _p(fr, _u16p)))
        return cls(cum, fr, h.size)

    @classmethod
    def uniform(cls, n_symbols: int = 256) -> "FrequencyTable":
        return cls.from_histogram(np.zeros(n_symbols, np.uint32))  # total == 0 -> uniform(n) (src/rans.rs:106-109)

    def get_symbol(self, sym: int) -> "RansSymbol":               # src/rans.rs:194
        if not 0 <= sym < self._n:
            raise IndexError("symbol index out of range")          # the reference panics
        return RansSymbol(int(self.cum_freq[sym]), int(self.freq[sym]))

    def __len__(self): return self._n

    def is_empty(self) -> bool: return self._n == 0


class RansSymbol:
    """reference src/rans.rs:59-72"""

    def __init__(self, cum_freq: int, freq: int):
        self.cum_freq = int(cum_freq) & 0xFFFF
        self.freq = int(freq) & 0xFFFF


class RansEncoder:
    """reference src/rans.rs:238-309: an encoder object; encode / encode_symbols any number of times, then finish."""

    def __init__(self):
        lib = load_library()
        self._h = lib.alice_codec_rans_encoder_new()
        if not self._h:
            _raise_last()

    @classmethod
    def with_capacity(cls, capacity: int): return cls()            # the capacity is a hint in the reference too

    def __del__(self):
        if getattr(self, "_h", None):
            load_library().alice_codec_rans_encoder_destroy(self._h)
            self._h = None

    def encode(self, sym: RansSymbol) -> None:                     # :269-285
        _check(load_library().alice_codec_rans_encoder_encode(self._h, sym.cum_freq, sym.freq))

    def encode_symbols(self, symbols, table: FrequencyTable) -> None:   # :288-294
        s = _as_u8(symbols)
        if s.size:
            _check(load_library().alice_codec_rans_encoder_encode_symbols(self._h, _p(s, _u8p), s.size, _p(table.cum_freq, _u16p),
                                                                          _p(table.freq, _u16p)))

    @property
    def state(self) -> int: return int(load_library().alice_codec_rans_encoder_state(self._h))

    def finish(self) -> bytes:                                     # :298-308, consumes the encoder
        lib = load_library()
        n = C.c_uint64()
        h, self._h = self._h, None
        p = lib.alice_codec_rans_encoder_finish(h, C.byref(n))
        if not p:
            _raise_last()
        try:
            return _copy_out(p, n.value).tobytes()
        finally:
            lib.alice_codec_data_free64(p, n.value)


class RansDecoder:
    """reference src/rans.rs:321-389: a decoder object; decode / decode_n continue from the current position."""

    def __init__(self, data):
        d = _as_u8(data)
        z = C.cast(C.c_char_p(b""), _u8p)
        self._h = load_library().alice_codec_rans_decoder_new(_p(d, _u8p) if d.size else z, d.size)
        if not self._h:
            _raise_last()

    def __del__(self):
        if getattr(self, "_h", None):
            load_library().alice_codec_rans_decoder_destroy(self._h)
            self._h = None

    def decode_n(self, n: int, table: FrequencyTable) -> np.ndarray:    # :375-381
        out = np.zeros(n, np.uint8)
        z = C.cast(C.c_char_p(b""), _u8p)
        _check(load_library().alice_codec_rans_decoder_decode_n(self._h, n, _p(table.cum_freq, _u16p), _p(table.freq, _u16p),
                                                                _p(out, _u8p) if n else z))
        return out

    def decode(self, table: FrequencyTable) -> int:                # :351-371
        return int(self.decode_n(1, table)[0])

    def is_empty(self) -> bool:                                    # :385-389
        return bool(load_library().alice_codec_rans_decoder_is_empty(self._h))

    @property
    def state(self) -> int: return int(load_library().alice_codec_rans_decoder_state(self._h))

    @property
    def position(self) -> int: return int(load_library().alice_codec_rans_decoder_position(self._h))


class InterleavedRansEncoder:
    """reference src/rans.rs:393-456: four interleaved streams (an opt-in format; `.alc` v1 uses RansEncoder)."""

    def __init__(self): self._pending = None

    def encode(self, symbols, table: FrequencyTable) -> None:
        self._pending = (_as_u8(symbols).copy(), table)

    def finish(self) -> bytes:
        lib = load_library()
        sym, table = self._pending if self._pending is not None else (np.zeros(0, np.uint8), FrequencyTable.uniform())
        n = C.c_uint64()
        z = C.cast(C.c_char_p(b""), _u8p)
        p = lib.alice_codec_rans_encode_interleaved(_p(sym, _u8p) if sym.size else z, sym.size, _p(table.cum_freq, _u16p),
                                                    _p(table.freq, _u16p), C.byref(n))
        if not p:
            _raise_last()
        try:
            return _copy_out(p, n.value).tobytes()
        finally:
            lib.alice_codec_data_free64(p, n.value)


class InterleavedRansDecoder:
    """reference src/rans.rs:468-519 (SimdRansDecoder, :531-666, decodes the same format to the same symbols)."""

    def __init__(self, data): self._data = _as_u8(data).copy()

    def decode_n(self, n: int, table: FrequencyTable) -> np.ndarray:
        out = np.zeros(n, np.uint8)
        z = C.cast(C.c_char_p(b""), _u8p)
        _check(load_library().alice_codec_rans_decode_interleaved(_p(self._data, _u8p) if self._data.size else z, self._data.size,
                                                                  _p(table.cum_freq, _u16p), _p(table.freq, _u16p), n,
                                                                  _p(out, _u8p) if n else z))
        return out


SimdRansDecoder = InterleavedRansDecoder


# ---------------------------------------------------------------------------------------------
# colour
# ---------------------------------------------------------------------------------------------

def rgb_bytes_to_ycocg_r(rgb):
    r = _as_u8(rgb)
    n = r.size // 3
    y = np.zeros(n, np.int16); co = np.zeros(n, np.int16); cg = np.zeros(n, np.int16)
    z = C.cast(C.c_char_p(b""), _u8p)
    _check(load_library().alice_codec_rgb_to_ycocg_r(_p(r, _u8p) if r.size else z, r.size, _p(y, _i16p), _p(co, _i16p), _p(cg, _i16p), n))
    return y, co, cg


def ycocg_r_to_rgb_bytes(y, co, cg) -> np.ndarray:
    y = np.ascontiguousarray(y, np.int16); co = np.ascontiguousarray(co, np.int16); cg = np.ascontiguousarray(cg, np.int16)
    if not (y.size == co.size == cg.size):
        raise CodecError(1, "channel lengths differ")
    out = np.zeros(y.size * 3, np.uint8)
    _check(load_library().alice_codec_ycocg_r_to_rgb(_p(y, _i16p), _p(co, _i16p), _p(cg, _i16p), y.size, _p(out, _u8p), out.size))
    return out


# ---------------------------------------------------------------------------------------------
# device-resident batches (inputs/outputs are device pointers, e.g. torch tensors' data_ptr())
# ---------------------------------------------------------------------------------------------

class Batch:
    """n_chunks equal-shaped chunks encoded/decoded entirely in HBM (alice_codec_batch_*)."""

    def __init__(self, width: int, height: int, frames: int, n_chunks: int, quality: int,
                 wavelet_type: WaveletType = WaveletType.Cdf53):
        lib = load_library()
        self.width, self.height, self.frames, self.n_chunks = width, height, frames, n_chunks
        self._h = lib.alice_codec_batch_create(width, height, frames, n_chunks, quality, int(wavelet_type))
        if not self._h:
            _raise_last()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.alice_codec_batch_destroy(h)

    def encode(self, d_rgb_ptr: int, stream: int = 0) -> None:
        _check(load_library().alice_codec_batch_encode(self._h, d_rgb_ptr, stream))

    def predict_sizes(self, d_rgb_ptr: int, stream: int = 0) -> "SizePrediction":
        """The size bracket of every chunk at every quality: arrays of shape (n_chunks, 101) (see predict_sizes)."""
        n = self.n_chunks
        lo = np.zeros((n, 101), np.uint64); hi = np.zeros_like(lo); st = np.zeros(lo.shape, np.uint8)
        _check(load_library().alice_codec_batch_predict_sizes(self._h, d_rgb_ptr, _p(lo, _u64p), _p(hi, _u64p), _p(st, _u8p), stream))
        return SizePrediction(lo, hi, st)

    def set_qualities(self, qualities=None) -> None:
        """One quality per chunk for the next encodes; None: the batch's own quality for every chunk again."""
        if qualities is None:
            _check(load_library().alice_codec_batch_set_qualities(self._h, None))
            return
        q = np.ascontiguousarray(qualities, np.int64).reshape(-1)
        if q.size != self.n_chunks or q.min() < 0 or q.max() > 255:
            raise ValueError(f"need {self.n_chunks} qualities in 0..255")
        q8 = q.astype(np.uint8)
        _check(load_library().alice_codec_batch_set_qualities(self._h, _p(q8, _u8p)))

    def encode_to_budget(self, d_rgb_ptr: int, budgets, min_quality: int = 10, max_quality: int = 95, stream: int = 0) -> tuple:
        """Each chunk once, at the highest quality whose predicted .alc length fits its budget (finish with
        encode_finish).  Returns (chosen qualities, fits) as numpy arrays; the chosen qualities stay set."""
        b = [int(x) for x in np.asarray(budgets, dtype=object).reshape(-1)]
        if len(b) != self.n_chunks:
            raise ValueError(f"need {self.n_chunks} budgets")
        _check_budget_args(b, min_quality, max_quality)
        bb = np.array(b, np.uint64)
        chosen = np.zeros(self.n_chunks, np.uint8); fits = np.zeros(self.n_chunks, np.uint8)
        _check(load_library().alice_codec_batch_encode_to_budget(self._h, d_rgb_ptr, _p(bb, _u64p), int(min_quality),
                                                                 int(max_quality), _p(chosen, _u8p), _p(fits, _u8p), stream))
        return chosen, fits.astype(bool)

    def encode_finish(self) -> np.ndarray:
        sizes = np.zeros(self.n_chunks, np.uint64)
        _check(load_library().alice_codec_batch_encode_finish(self._h, _p(sizes, _u64p)))
        return sizes

    def alc_ptr(self, chunk: int = 0) -> int:
        return load_library().alice_codec_batch_alc_ptr(self._h, chunk)

    @property
    def alc_stride(self) -> int:
        return load_library().alice_codec_batch_alc_stride(self._h)

    def pack_alc(self, sizes: np.ndarray, d_dst_ptr: int, dst_capacity: int, stream: int = 0) -> None:
        sizes = np.ascontiguousarray(sizes, np.uint64)
        _check(load_library().alice_codec_batch_pack_alc(self._h, _p(sizes, _u64p), d_dst_ptr, dst_capacity, stream))

    def decode(self, d_alc_ptr: int, alc_stride: int, d_rgb_out_ptr: int | None, stream: int = 0) -> None:
        """d_rgb_out_ptr None: decode into the batch's own storage, read the pixels at rgb_ptr(chunk)."""
        _check(load_library().alice_codec_batch_decode(self._h, d_alc_ptr, alc_stride, d_rgb_out_ptr, stream))

    def decode_finish(self) -> None:
        _check(load_library().alice_codec_batch_decode_finish(self._h))

    def _origins(self, origins) -> np.ndarray:
        o = [[_u32_arg(v, "origin") for v in xy] for xy in origins]
        if len(o) != self.n_chunks or any(len(xy) != 2 for xy in o):
            raise CodecError(1, f"origins: expected {self.n_chunks} (x, y) pairs")
        return np.array(o, np.uint32).reshape(-1)

    def encode_regions(self, d_frames_ptr: int, frame_width: int, frame_height: int, origins, stream: int = 0) -> None:
        """chunk i = frames [i*frames, (i+1)*frames) of d_frames (frame_width x frame_height RGB), cropped to the batch's
        width x height at origins[i] = (x, y) in pixels; the .alc equals FrameEncoder.encode of that crop."""
        o = self._origins(origins)
        _check(load_library().alice_codec_batch_encode_regions(self._h, d_frames_ptr, _u32_arg(frame_width, "frame_width"),
                                                               _u32_arg(frame_height, "frame_height"), _p(o, _u32p), stream))

    def decode_regions(self, d_alc_ptr: int, alc_stride: int, d_frames_out_ptr: int, frame_width: int, frame_height: int,
                       origins, stream: int = 0) -> None:
        """decodes chunk i into its rectangle of d_frames_out; bytes outside the rectangles are not written"""
        o = self._origins(origins)
        _check(load_library().alice_codec_batch_decode_regions(self._h, d_alc_ptr, alc_stride, d_frames_out_ptr,
                                                               _u32_arg(frame_width, "frame_width"),
                                                               _u32_arg(frame_height, "frame_height"), _p(o, _u32p), stream))

    def stage_ms(self) -> dict:
        out = (C.c_float * 6)()
        load_library().alice_codec_batch_stage_ms(self._h, out)
        keys = ["forward_transform", "rans_table", "rans_encode", "assemble", "rans_decode", "inverse_transform"]
        return dict(zip(keys, [float(v) for v in out]))

    def rgb_ptr(self, chunk: int = 0) -> int:
        return load_library().alice_codec_batch_rgb_ptr(self._h, chunk)

    def symbols_ptr(self) -> int:
        return load_library().alice_codec_batch_symbols_ptr(self._h)

    @property
    def padded_pixels(self) -> int:
        return load_library().alice_codec_batch_padded_pixels(self._h)

    @property
    def bytes_per_chunk(self) -> int:
        """device bytes the batch holds per chunk at its current .alc capacities (symbols, .alc buffer, tables)"""
        return load_library().alice_codec_batch_bytes_per_chunk(self._h)

    @property
    def fixed_bytes(self) -> int:
        """device bytes the batch holds whatever its chunk count (transform scratch)"""
        return load_library().alice_codec_batch_fixed_bytes(self._h)


# ---------------------------------------------------------------------------------------------
# person segmentation (reference src/segment.rs; kernels in csrc/segment.hip)
# ---------------------------------------------------------------------------------------------

_U32 = 0xFFFFFFFF


def _nz(a: np.ndarray, t):
    return _p(a, t) if a.size else C.cast(C.c_char_p(b"\0\0\0\0"), t)


def _u32_arg(v, what: str) -> int:
    v = int(v)
    if not 0 <= v <= _U32:
        raise CodecError(3, f"{what} out of u32 range")
    return v


class SegmentConfig:
    """reference src/segment.rs:42-63.  min_region_size is carried and, as in the reference, not used."""

    def __init__(self, motion_threshold: int = 25, min_region_size: int = 100, dilate_radius: int = 2, erode_radius: int = 1):
        self.motion_threshold = int(motion_threshold)
        self.min_region_size = int(min_region_size)
        self.dilate_radius = int(dilate_radius)
        self.erode_radius = int(erode_radius)

    def __repr__(self):
        return (f"SegmentConfig(motion_threshold={self.motion_threshold}, min_region_size={self.min_region_size}, "
                f"dilate_radius={self.dilate_radius}, erode_radius={self.erode_radius})")


class SegmentResult:
    """reference src/segment.rs:78-154: mask (u8, 1 = person), bbox [x, y, w, h], foreground_count, width, height."""

    def __init__(self, mask, bbox, foreground_count: int, width: int, height: int):
        self.mask = _as_u8(mask)
        self.bbox = [int(v) for v in bbox]
        self.foreground_count = int(foreground_count)
        self.width = int(width)
        self.height = int(height)

    def coverage(self) -> float:
        """f32 arithmetic as in :94-101 (count * (1 / total)); 0.0 for an empty frame."""
        total = self.width * self.height
        if total > _U32:
            raise CodecError(3, "width * height does not fit u32")
        if total == 0:
            return 0.0
        inv = np.float32(1.0) / np.float32(total)
        return float(np.float32(self.foreground_count) * inv)

    def extract_person_rgb(self, frame_rgb) -> bytes:
        """:107-125 -- the bbox pixels whose mask byte is exactly 1."""
        return extract_person_rgb(self.mask, self.width, self.bbox, frame_rgb)

    def rle_encode_mask(self) -> bytes:
        """:131-154 -- [len u16 LE, value u8] per run of (mask & 1)."""
        return rle_encode_mask(self.mask)


def _seg_out(rc: int, mask: np.ndarray, bbox: np.ndarray, count, width: int, height: int) -> SegmentResult:
    _check(rc)
    return SegmentResult(mask, [int(v) for v in bbox], int(count.value), width, height)


def segment_by_motion(current, reference, width: int, height: int, config: SegmentConfig | None = None) -> SegmentResult:
    """reference src/segment.rs:172-230 on the GPU."""
    cfg = config or SegmentConfig()
    w, h = _u32_arg(width, "width"), _u32_arg(height, "height")
    cur, ref = _as_u8(current), _as_u8(reference)
    total = w * h
    mask = np.zeros(total if total <= _U32 else 0, np.uint8)
    bbox = np.zeros(4, np.uint32)
    cnt = C.c_uint32()
    rc = load_library().alice_codec_segment_by_motion(_nz(cur, _u8p), cur.size, _nz(ref, _u8p), ref.size, w, h,
                                                      int(cfg.motion_threshold) & 0xFF, _u32_arg(cfg.dilate_radius, "dilate_radius"),
                                                      _u32_arg(cfg.erode_radius, "erode_radius"), _nz(mask, _u8p), mask.size,
                                                      _p(bbox, _u32p), C.byref(cnt))
    return _seg_out(rc, mask, bbox, cnt, w, h)


def segment_by_chroma(y, co, cg, width: int, height: int, green_threshold: int) -> SegmentResult:
    """reference src/segment.rs:234-265 on the GPU (y and co are accepted and ignored, as there).  A cg shorter than
    width*height raises InvalidBufferSize where the reference panics."""
    del y, co
    w, h = _u32_arg(width, "width"), _u32_arg(height, "height")
    c = np.ascontiguousarray(cg, np.int16).reshape(-1)
    total = w * h
    mask = np.zeros(total if total <= _U32 else 0, np.uint8)
    bbox = np.zeros(4, np.uint32)
    cnt = C.c_uint32()
    rc = load_library().alice_codec_segment_by_chroma(_nz(c, _i16p), c.size, w, h, int(green_threshold), _nz(mask, _u8p), mask.size,
                                                      _p(bbox, _u32p), C.byref(cnt))
    return _seg_out(rc, mask, bbox, cnt, w, h)


def rle_encode_mask(mask) -> bytes:
    """SegmentResult::rle_encode_mask (src/segment.rs:131-154) of any byte mask, on the GPU."""
    m = _as_u8(mask)
    lib = load_library()
    n = C.c_uint64()
    p = lib.alice_codec_rle_encode_mask(_nz(m, _u8p), m.size, C.byref(n))
    if not p:
        _raise_last()
    try:
        return _copy_out(p, n.value).tobytes()
    finally:
        lib.alice_codec_data_free64(p, n.value)


def extract_person_rgb(mask, width: int, bbox, frame_rgb) -> bytes:
    """SegmentResult::extract_person_rgb (src/segment.rs:107-125) on the GPU."""
    m, rgb = _as_u8(mask), _as_u8(frame_rgb)
    b = np.array([_u32_arg(v, "bbox") for v in bbox], np.uint32)
    out = np.zeros(3 * int(b[2]) * int(b[3]), np.uint8)
    n = C.c_uint64()
    _check(load_library().alice_codec_extract_person_rgb(_nz(m, _u8p), m.size, _u32_arg(width, "width"), _p(b, _u32p), _nz(rgb, _u8p),
                                                          rgb.size, _nz(out, _u8p), out.size, C.byref(n)))
    return out[:n.value].tobytes()


def _bbox_rows(frame_width: int, bbox):
    """rows of crop_to_bbox / paste_from_bbox (src/segment.rs:269-298): (start, end) per row; u32 row * frame_width + bx"""
    bx, by, bw, bh = (_u32_arg(v, "bbox") for v in bbox)
    fw = _u32_arg(frame_width, "frame_width")
    if by + bh > _U32:
        raise CodecError(3, "bbox y + h does not fit u32")
    for row in range(by, by + bh):
        start = row * fw + bx
        if start > _U32:
            raise CodecError(3, "row * frame_width + x does not fit u32")
        yield start, start + bw


def crop_to_bbox(frame, frame_width: int, bbox) -> bytes:
    """reference src/segment.rs:269-281 (host byte copy): a row whose end falls past the frame is skipped."""
    f = _as_u8(frame)
    bw = int(bbox[2])
    parts = [f[s:e] for s, e in _bbox_rows(frame_width, bbox) if e <= f.size]
    return np.concatenate(parts).tobytes() if parts and bw else b""


def paste_from_bbox(frame: np.ndarray, frame_width: int, person_data, bbox) -> np.ndarray:
    """reference src/segment.rs:284-298 (host byte copy) into `frame` (a writable uint8 array), which is returned."""
    if not (isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.flags.c_contiguous):
        raise TypeError("frame must be a C-contiguous uint8 numpy array")
    dst = frame.reshape(-1)
    src = _as_u8(person_data)
    bw = int(bbox[2])
    off = 0
    for s, e in _bbox_rows(frame_width, bbox):
        if e <= dst.size and off + bw <= src.size:
            dst[s:e] = src[off:off + bw]
        off += bw
    return frame


# the reference's own Python functions (src/python.rs:80-267): same names, arguments, defaults and return shapes;
# frames are 2-D [H, W] arrays

def _plane(a, dtype) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("expected a 2-D [H, W] array")
    return np.ascontiguousarray(a, dtype)


def segment_motion_numpy(current, reference, motion_threshold: int = 25, dilate_radius: int = 2, erode_radius: int = 1):
    """-> (mask [H, W] uint8, [x, y, w, h], foreground_count)  (src/python.rs:80-129)"""
    cur, ref = _plane(current, np.uint8), _plane(reference, np.uint8)
    h, w = cur.shape
    r = segment_by_motion(cur, ref, w, h, SegmentConfig(motion_threshold, 100, dilate_radius, erode_radius))
    return r.mask.reshape(h, w), r.bbox, r.foreground_count


def segment_chroma_numpy(y_channel, co_channel, cg_channel, green_threshold: int = 30):
    """-> (mask [H, W] uint8, [x, y, w, h], foreground_count)  (src/python.rs:141-184; shape from the Y plane)"""
    h, w = _plane(y_channel, np.int16).shape
    r = segment_by_chroma(None, None, _plane(cg_channel, np.int16), w, h, green_threshold)
    return r.mask.reshape(h, w), r.bbox, r.foreground_count


def crop_bbox_numpy(frame, bbox) -> np.ndarray:
    """-> [bh, bw] uint8  (src/python.rs:195-217)"""
    if len(bbox) != 4:
        raise ValueError("bbox must have 4 elements")
    f = _plane(frame, np.uint8)
    out = np.frombuffer(crop_to_bbox(f, f.shape[1], bbox), np.uint8).copy()
    return out.reshape(int(bbox[3]), int(bbox[2]))


def paste_bbox_numpy(frame: np.ndarray, person_data, bbox) -> None:
    """in place into a C-contiguous [H, W] uint8 frame  (src/python.rs:227-248)"""
    if len(bbox) != 4:
        raise ValueError("bbox must have 4 elements")
    if not (isinstance(frame, np.ndarray) and frame.ndim == 2):
        raise ValueError("expected a 2-D [H, W] array")
    paste_from_bbox(frame, frame.shape[1], person_data, bbox)


def rle_encode_numpy(mask) -> list:
    """-> list of byte values, as PyO3 returns a Vec<u8>  (src/python.rs:257-271)"""
    return list(rle_encode_mask(_plane(mask, np.uint8)))


# device-resident (data_ptr() integers, like Batch); stats = n_frames x {x, y, w, h, count} uint32

def segment_motion_device(d_current: int, d_reference: int, reference_stride: int, width: int, height: int, n_frames: int,
                          d_stats: int, d_mask: int | None = None, config: SegmentConfig | None = None, stream: int = 0) -> None:
    cfg = config or SegmentConfig()
    _check(load_library().alice_codec_dev_segment_motion(d_current, d_reference, reference_stride, width, height, n_frames,
                                                         int(cfg.motion_threshold) & 0xFF, cfg.dilate_radius, cfg.erode_radius,
                                                         d_mask, d_stats, stream))


def segment_chroma_rgb_device(d_rgb: int, width: int, height: int, n_frames: int, green_threshold: int, d_stats: int,
                              d_mask: int | None = None, stream: int = 0) -> None:
    _check(load_library().alice_codec_dev_segment_chroma_rgb(d_rgb, width, height, n_frames, int(green_threshold), d_mask, d_stats,
                                                             stream))


def rle_bound(n: int) -> int:
    return int(load_library().alice_codec_rle_bound(n))


def rle_encode_mask_device(d_mask: int, n: int, d_out: int, cap: int, stream: int = 0) -> int:
    """-> bytes written at d_out (cap >= rle_bound(n))"""
    out = C.c_uint64()
    _check(load_library().alice_codec_dev_rle_encode_mask(d_mask, n, d_out, cap, C.byref(out), stream))
    return out.value


def extract_person_rgb_device(d_mask: int, width: int, height: int, bbox, d_rgb: int, d_out: int, cap: int, stream: int = 0) -> int:
    """-> bytes written at d_out (cap >= 3 * bbox w * h)"""
    b = np.array([_u32_arg(v, "bbox") for v in bbox], np.uint32)
    out = C.c_uint64()
    _check(load_library().alice_codec_dev_extract_person_rgb(d_mask, width, height, _p(b, _u32p), d_rgb, d_out, cap, C.byref(out),
                                                             stream))
    return out.value


# ---------------------------------------------------------------------------------------------
# hybrid streaming (reference src/segment.rs:1-8, README "Person Segmentation"): only the person's box is coded, and the
# decoder pastes it back over a background.  Segmentation, crop, encode, decode and paste all run in HBM: the region calls
# of Batch read and write the boxes of the full frames in place, and only the 20 B/frame stats come to the host.
# ---------------------------------------------------------------------------------------------

def _dptr(x) -> int:
    """a device pointer: an int, or anything with data_ptr() (a torch tensor)"""
    return int(x) if isinstance(x, int) else int(x.data_ptr())


def _positive_u32(v, what: str) -> int:
    v = _u32_arg(v, what)
    if v == 0:
        raise CodecError(2, f"{what} must be positive")
    return v


def person_chunk_boxes(stats, width: int, height: int, frames: int) -> list:
    """The box policy of encode_person_chunks: [x, y, w, h] in pixels per chunk, from the per-frame segmentation stats
    (n_chunks * frames rows of {x, y, w, h, count}, pixel units).  A chunk whose frames have no foreground gets
    [0, 0, 0, 0].  All others share one w x h, and each box contains its chunk's union box and lies inside the frame.
    Where width % 4 == 0 every x is a multiple of 4 (the tile kernels' dword path) and so is the common width, which keeps
    a box pushed against the right edge on a multiple of 4: the common width is the widest span from a union box's
    4-aligned left edge to its right edge, rounded up to 4 (at most 6 more than the widest union box), clamped to the
    frame width."""
    W, H, f = _positive_u32(width, "width"), _positive_u32(height, "height"), _positive_u32(frames, "frames")
    st = np.asarray(stats, dtype=np.int64)
    if st.ndim != 2 or st.shape[1] != 5 or st.shape[0] % f:
        raise CodecError(1, f"stats: expected n_chunks * {f} rows of {{x, y, w, h, count}}, got shape {st.shape}")
    unions = []
    for c in range(st.shape[0] // f):
        s = st[c * f:(c + 1) * f]
        s = s[s[:, 4] > 0]
        if not len(s):
            unions.append(None)
            continue
        u = (int(s[:, 0].min()), int(s[:, 1].min()), int((s[:, 0] + s[:, 2]).max()), int((s[:, 1] + s[:, 3]).max()))
        if u[0] < 0 or u[1] < 0 or u[2] > W or u[3] > H:
            raise CodecError(2, f"chunk {c}: foreground box {u} does not lie inside the {W}x{H} frame")
        unions.append(u)
    fg = [u for u in unions if u is not None]
    if not fg:
        return [[0, 0, 0, 0] for _ in unions]
    align = W % 4 == 0
    if align:
        cw = min(W, (max(x1 - (x0 & ~3) for x0, _, x1, _ in fg) + 3) & ~3)
    else:
        cw = max(x1 - x0 for x0, _, x1, _ in fg)
    ch = max(y1 - y0 for _, y0, _, y1 in fg)
    boxes = []
    for u in unions:
        if u is None:
            boxes.append([0, 0, 0, 0])
            continue
        x = min(u[0], W - cw)
        boxes.append([x & ~3 if align else x, min(u[1], H - ch), cw, ch])
    return boxes


def _runs(boxes) -> list:
    """maximal runs [start, end) of consecutive chunks with the same non-empty box size: one Batch call each"""
    out, i = [], 0
    while i < len(boxes):
        if boxes[i][2] * boxes[i][3] == 0:
            i += 1
            continue
        j = i + 1
        while j < len(boxes) and boxes[j][2:] == boxes[i][2:]:
            j += 1
        out.append((i, j))
        i = j
    return out


def encode_person_chunks(d_frames, d_background, width: int, height: int, frames: int, n_chunks: int, quality: int,
                         wavelet: WaveletType = WaveletType.Cdf53, config: SegmentConfig | None = None,
                         green_threshold: int | None = None, format: str = "v1", lane_symbols: int = 0,
                         max_bytes: int | None = None, min_psnr: float | None = None) -> list:
    """Hybrid encode of n_chunks chunks of `frames` frames each (d_frames: n_chunks * frames frames of width x height
    interleaved RGB in HBM) -> list of (bbox [x, y, w, h] in pixels, .alc bytes), one per chunk.

    1. Segmentation of all frames in one call.  Motion (default): against the one background frame d_background (RGB of
       the same shape), on the interleaved bytes as a (3 * width)-sample row, so a pixel is foreground when any of its
       channels moved; config's radii then count bytes along a row and rows down a column.  green_threshold given:
       chroma keying of the RGB frames instead (segment_chroma_rgb_device), d_background unused.
    2. Per chunk the union of its frames' boxes (only the stats come to the host), 3. person_chunk_boxes, 4. Batch region
       encodes of the chunks with foreground (one per run of consecutive such chunks).  A chunk without foreground gets
       bbox [0, 0, 0, 0] and the reference's empty chunk, FrameEncoder.encode(b"", 0, 0, frames).

    format="split" codes the boxes as version 2 (split_encode_regions_device; lane_symbols 0: the default), with the
    version 2 empty chunk for chunks without foreground; format="wide" does the same with version 3
    (wide_encode_regions_device), the container to choose for qualities above about 90.  max_bytes (split and wide only) is
    a byte budget per chunk: every box is then coded at the quality split_encode_to_budget_device /
    wide_encode_to_budget_device picks in [min(10, hi), hi], hi = min(quality, 100), and a chunk that cannot be guaranteed
    to fit is coded at the low end of the range.  format="reversible" codes the boxes as version 4
    (reversible_encode_regions_device): at quality 100 the boxes come back exactly; it has no byte budget.  min_psnr (split
    and wide only, not together with max_bytes) is a PSNR floor in dB per chunk, measured on the box: every box is coded at
    the lowest quality in [min(10, hi), hi] that split_encode_to_psnr_device / wide_encode_to_psnr_device finds to reach it,
    and at hi when none does."""
    if format not in ("v1", "split", "wide", "reversible"):
        raise CodecError(9, f"format must be 'v1', 'split', 'wide' or 'reversible', got {format!r}")
    if min_psnr is not None and max_bytes is not None:
        raise CodecError(9, "min_psnr and max_bytes are two rate controls: give one of them")
    if min_psnr is not None and format not in ("split", "wide"):
        raise CodecError(9, "min_psnr is a version 2 / version 3 quality floor: it needs format='split' or format='wide' "
                            "(version 1 has no quality to control, and a lossless encode has no quality to search)")
    if min_psnr is not None:
        min_psnr = _check_min_psnr(min_psnr)
    if max_bytes is not None and format not in ("split", "wide"):
        raise CodecError(9, "max_bytes is a version 2 / version 3 budget: it needs format='split' or format='wide'")
    W, H, f = _positive_u32(width, "width"), _positive_u32(height, "height"), _positive_u32(frames, "frames")
    n = _positive_u32(n_chunks, "n_chunks")
    if not 0 <= int(quality) <= 255:
        raise CodecError(5, f"quality must fit a u8, got {quality}")
    wavelet = WaveletType(wavelet)
    cfg = config or SegmentConfig()
    if n * f > _U32 or 3 * W > _U32:
        raise CodecError(3, "n_chunks * frames and 3 * width must fit u32")
    if green_threshold is None and d_background is None:
        raise CodecError(9, "motion segmentation needs d_background")
    import torch
    frames_ptr = _dptr(d_frames)
    stats = torch.zeros(n * f * 5, dtype=torch.int32, device="cuda")
    if green_threshold is None:
        segment_motion_device(frames_ptr, _dptr(d_background), 0, 3 * W, H, n * f, stats.data_ptr(), config=cfg)
        torch.cuda.synchronize()
        st = stats.cpu().numpy().view(np.uint32).reshape(-1, 5).astype(np.int64)
        x0, x1 = st[:, 0] // 3, -(-(st[:, 0] + st[:, 2]) // 3)          # byte columns -> the pixels they belong to
        st[:, 0], st[:, 2] = x0, x1 - x0
    else:
        segment_chroma_rgb_device(frames_ptr, W, H, n * f, int(green_threshold), stats.data_ptr())
        torch.cuda.synchronize()
        st = stats.cpu().numpy().view(np.uint32).reshape(-1, 5).astype(np.int64)
    boxes = person_chunk_boxes(st, W, H, f)
    frame_bytes = W * H * 3
    if format in ("split", "wide", "reversible"):
        wide = format != "split"
        enc = FrameEncoder(int(quality), wavelet)
        empty = {"split": encode_split, "wide": encode_wide, "reversible": encode_reversible}[format](enc, b"", 0, 0, f, lane_symbols)
        bound = wide_stream_bound if wide else split_stream_bound
        encode_regions = {"split": split_encode_regions_device, "wide": wide_encode_regions_device,
                          "reversible": reversible_encode_regions_device}[format]
        encode_to_budget = wide_encode_to_budget_device if wide else split_encode_to_budget_device   # (max_bytes: split, wide)
        encode_to_psnr = wide_encode_to_psnr_device if wide else split_encode_to_psnr_device         # (min_psnr: split, wide)
        out = [(b, empty) for b in boxes]
        for i, j in _runs(boxes):
            bw, bh = boxes[i][2], boxes[i][3]
            stride = (SPLIT_HEADER_BYTES + 3 * bound(_padded_pixels(bw, bh, f), lane_symbols or SPLIT_DEFAULT_LANE_SYMBOLS)
                      + 255) & ~255
            d_out = torch.empty((j - i) * stride, dtype=torch.uint8, device="cuda")
            origins = [b[:2] for b in boxes[i:j]]
            src = frames_ptr + i * f * frame_bytes
            if min_psnr is not None:
                hi_q = min(int(quality), 100)
                _, _, _, sizes = encode_to_psnr(src, bw, bh, f, j - i, wavelet, min_psnr, d_out.data_ptr(), stride,
                                                min_quality=min(10, hi_q), max_quality=hi_q, lane_symbols=lane_symbols,
                                                frame_width=W, frame_height=H, origins=origins)
            elif max_bytes is None:
                sizes = encode_regions(src, W, H, origins, bw, bh, f, wavelet, int(quality), d_out.data_ptr(), stride,
                                       lane_symbols=lane_symbols)
            else:
                hi_q = min(int(quality), 100)
                _, _, sizes = encode_to_budget(src, bw, bh, f, j - i, wavelet, [int(max_bytes)] * (j - i),
                                               d_out.data_ptr(), stride, min_quality=min(10, hi_q), max_quality=hi_q,
                                               lane_symbols=lane_symbols, frame_width=W, frame_height=H, origins=origins)
            host = d_out.cpu().numpy().reshape(j - i, stride)
            for k in range(j - i):
                out[i + k] = (boxes[i + k], host[k, :int(sizes[k])].tobytes())
        return out
    empty = FrameEncoder(int(quality), wavelet).encode(b"", 0, 0, f).to_bytes()
    out = [(b, empty) for b in boxes]
    batches = {}
    for i, j in _runs(boxes):
        bw, bh = boxes[i][2], boxes[i][3]
        key = (bw, bh, j - i)
        if key not in batches:
            batches[key] = Batch(bw, bh, f, j - i, int(quality), wavelet)
        batch = batches[key]
        batch.encode_regions(frames_ptr + i * f * frame_bytes, W, H, [b[:2] for b in boxes[i:j]])
        sizes = batch.encode_finish()
        packed = torch.empty(int(sizes.sum()), dtype=torch.uint8, device="cuda")
        batch.pack_alc(sizes, packed.data_ptr(), packed.numel())
        torch.cuda.synchronize()
        host = packed.cpu().numpy()
        ends = np.cumsum(sizes.astype(np.int64))
        for k in range(j - i):
            out[i + k] = (boxes[i + k], host[ends[k] - int(sizes[k]):ends[k]].tobytes())
    return out


def decode_person_chunks(chunks, d_frames_out, width: int, height: int, frames: int) -> None:
    """Hybrid decode: chunk k of `chunks` (encode_person_chunks' list of (bbox, .alc bytes)) is decoded and pasted into
    its bbox of frames [k * frames, (k + 1) * frames) of d_frames_out (width x height RGB in HBM, typically holding the
    background).  Empty chunks paste nothing; no byte outside the boxes is written.  Each chunk is decoded by its own
    container version (alc_version), so a list may mix chunks of versions 1 to 4."""
    W, H, f = _positive_u32(width, "width"), _positive_u32(height, "height"), _positive_u32(frames, "frames")
    boxes, alcs, versions, lanes = [], [], [], {}
    for k, (bbox, alc) in enumerate(chunks):
        b = [_u32_arg(v, "bbox") for v in bbox]
        if len(b) != 4:
            raise CodecError(2, f"chunk {k}: bbox must have 4 elements")
        if b[2] * b[3] and (b[0] + b[2] > W or b[1] + b[3] > H):
            raise CodecError(2, f"chunk {k}: bbox {b} does not lie inside the {W}x{H} frame")
        data = bytes(alc)
        version = alc_version(data)
        if b[2] * b[3]:
            c = (split_info(data) if version == 2 else wide_info(data) if version == 3 else reversible_info(data) if version == 4
                 else EncodedChunk.from_bytes(data))
            if (c.width, c.height, c.frames) != (b[2], b[3], f):
                raise CodecError(2, f"chunk {k}: .alc is {c.width}x{c.height}x{c.frames}, bbox says {b[2]}x{b[3]}x{f}")
            if version in (2, 3, 4):
                lanes[k] = c.lane_symbols
        boxes.append(b)
        alcs.append(data)
        versions.append(version)
    # one device call per run of consecutive chunks of one box size, one container version and one lane_symbols
    runs = []
    for i, j in _runs(boxes):
        s0 = i
        for k in range(i + 1, j + 1):
            if k == j or (versions[k], lanes.get(k)) != (versions[s0], lanes.get(s0)):
                runs.append((s0, k))
                s0 = k
    if not runs:
        return
    import torch
    out_ptr = _dptr(d_frames_out)
    frame_bytes = W * H * 3
    batches = {}
    for i, j in runs:
        bw, bh = boxes[i][2], boxes[i][3]
        if versions[i] in (2, 3, 4):
            decode_regions = {2: split_decode_regions_device, 3: wide_decode_regions_device,
                              4: reversible_decode_regions_device}[versions[i]]
            stride = (max(len(a) for a in alcs[i:j]) + 255) & ~255
            host = np.zeros((j - i, stride), np.uint8)
            for k in range(i, j):
                host[k - i, :len(alcs[k])] = np.frombuffer(alcs[k], np.uint8)
            d_alc = torch.from_numpy(host).to("cuda")
            decode_regions(d_alc.data_ptr(), stride, [len(a) for a in alcs[i:j]], out_ptr + i * f * frame_bytes, W, H,
                           [b[:2] for b in boxes[i:j]])
            continue
        stride = (max(len(a) for a in alcs[i:j]) + 255) & ~255
        host = np.zeros((j - i, stride), np.uint8)
        for k in range(i, j):
            host[k - i, :len(alcs[k])] = np.frombuffer(alcs[k], np.uint8)
        d_alc = torch.from_numpy(host).to("cuda")
        key = (bw, bh, j - i)
        if key not in batches:
            batches[key] = Batch(bw, bh, f, j - i, 90)
        batch = batches[key]
        batch.decode_regions(d_alc.data_ptr(), stride, out_ptr + i * f * frame_bytes, W, H, [b[:2] for b in boxes[i:j]])
        batch.decode_finish()


# ---- split-stream format (.alc version 2) ----
# v1 is the format for byte compatibility with the reference; v2 is for video that comes back and for the latency of one chunk.

SPLIT_DEFAULT_LANE_SYMBOLS = 512
SPLIT_HEADER_BYTES = 1630


class _CSplitInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("frames", C.c_uint32), ("lane_symbols", C.c_uint32),
                ("wavelet", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("quant_step", C.c_int32 * 3), ("dead_zone", C.c_int32 * 3),
                ("num_symbols", C.c_uint32 * 3), ("n_blocks", C.c_uint32 * 3), ("payload_len", C.c_uint64 * 3)]


class SplitInfo:
    """The header fields of a version 2 container (alice_codec_split_info: validated, no device needed)."""

    def __init__(self, c: _CSplitInfo):
        self.width, self.height, self.frames = int(c.width), int(c.height), int(c.frames)
        self.lane_symbols = int(c.lane_symbols)
        self.wavelet_type = WaveletType(int(c.wavelet))
        self.quant_step = [int(v) for v in c.quant_step]
        self.dead_zone = [int(v) for v in c.dead_zone]
        self.num_symbols = [int(v) for v in c.num_symbols]
        self.n_blocks = [int(v) for v in c.n_blocks]
        self.payload_len = [int(v) for v in c.payload_len]

    def __repr__(self):
        return (f"SplitInfo({self.width}x{self.height}x{self.frames}, {self.wavelet_type.name}, lane_symbols={self.lane_symbols}, "
                f"steps={self.quant_step}, blocks={self.n_blocks}, payload={self.payload_len})")


def split_info(data) -> SplitInfo:
    buf = _as_u8(data)
    c = _CSplitInfo()
    _check(load_library().alice_codec_split_info(_p(buf, _u8p), buf.size, C.byref(c)))
    return SplitInfo(c)


def alc_version(data) -> int:
    """The version byte of a container (0 when the data is too short to have one)."""
    buf = _as_u8(data)
    return int(buf[4]) if buf.size > 4 else 0


def encode_split(encoder: "FrameEncoder", rgb_frames, width: int, height: int, frames: int, lane_symbols: int = 0) -> bytes:
    """One chunk as version 2 bytes, with the encoder's wavelet and quality (lane_symbols 0: the default)."""
    lib = load_library()
    buf = _as_u8(rgb_frames)
    _dims_u32(width, height, frames, lane_symbols)
    n = C.c_uint64(0)
    src = _p(buf, _u8p) if buf.size else C.cast(C.c_char_p(b""), _u8p)
    ptr = lib.alice_codec_encode_split(encoder._h, src, buf.size, width, height, frames, lane_symbols, C.byref(n))
    if not ptr:
        _raise_last()
    try:
        return _copy_out(ptr, n.value).tobytes()
    finally:
        lib.alice_codec_data_free64(ptr, n.value)


def decode_split(data) -> np.ndarray:
    """The RGB bytes of a version 2 container."""
    lib = load_library()
    buf = _as_u8(data)
    n = C.c_uint64(0)
    ptr = lib.alice_codec_decode_split(_p(buf, _u8p), buf.size, C.byref(n))
    if not ptr:
        _raise_last()
    return _adopt(ptr, n.value, lib.alice_codec_data_free64)


def normalized_frequencies(histogram) -> np.ndarray:
    """The 256 frequencies a version 2 header stores for this histogram (sum 4096), from the table kernel."""
    h = np.ascontiguousarray(histogram, dtype=np.uint32).reshape(-1)
    if h.size != 256:
        raise ValueError("histogram must have 256 bins")
    f = np.zeros(256, np.uint16)
    _check(load_library().alice_codec_split_normalize(_p(h, _u32p), _p(f, _u16p)))
    return f


def split_stream_bound(n: int, lane_symbols: int = SPLIT_DEFAULT_LANE_SYMBOLS) -> int:
    return int(load_library().alice_codec_split_stream_bound(n, lane_symbols))


def split_encode_device(d_rgb_ptr: int, width: int, height: int, frames: int, n_chunks: int, wavelet_type: WaveletType,
                        quality: int, d_out_ptr: int, out_stride: int, qualities=None, lane_symbols: int = 0,
                        stream: int = 0) -> np.ndarray:
    """n_chunks packed device chunks -> version 2 bytes at d_out_ptr + i * out_stride; returns the sizes."""
    sizes = np.zeros(n_chunks, np.uint64)
    q = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8).reshape(-1)
    if q is not None and q.size != n_chunks:
        raise ValueError("one quality per chunk")
    _dims_u32(width, height, frames, n_chunks, lane_symbols)
    _check(load_library().alice_codec_dev_encode_split(d_rgb_ptr, width, height, frames, n_chunks, int(wavelet_type), quality,
                                                       None if q is None else _p(q, _u8p), lane_symbols, d_out_ptr, out_stride,
                                                       _p(sizes, _u64p), stream or None))
    return sizes


def split_decode_device(d_alc_ptr: int, alc_stride: int, sizes, d_rgb_out_ptr: int, stream: int = 0) -> None:
    s = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    _check(load_library().alice_codec_dev_decode_split(d_alc_ptr, alc_stride, _p(s, _u64p), s.size, d_rgb_out_ptr, stream or None))


def _padded_pixels(width: int, height: int, frames: int) -> int:
    """Symbols per channel of a width x height x frames chunk: every side padded to even, one frame to two."""
    if width * height * frames == 0:
        return 0
    return (width + (width & 1)) * (height + (height & 1)) * (2 if frames == 1 else frames + (frames & 1))


# ---- wide format (.alc version 3) ----
# Version 2 with an untruncated symbol: the format for the top of the quality scale, where versions 1 and 2 wrap large
# coefficients modulo 256.  lane_symbols: a power of two in [64, 8192].  No size prediction, budgets or regions yet.

WIDE_MAX_LANE_SYMBOLS = 8192


def wide_info(data) -> SplitInfo:
    """The header fields of a version 3 container (validated, no device needed); the fields are version 2's."""
    buf = _as_u8(data)
    c = _CSplitInfo()
    _check(load_library().alice_codec_wide_info(_p(buf, _u8p), buf.size, C.byref(c)))
    return SplitInfo(c)


def encode_wide(encoder: "FrameEncoder", rgb_frames, width: int, height: int, frames: int, lane_symbols: int = 0) -> bytes:
    """One chunk as version 3 bytes, with the encoder's wavelet and quality (lane_symbols 0: the default)."""
    lib = load_library()
    buf = _as_u8(rgb_frames)
    _dims_u32(width, height, frames, lane_symbols)
    n = C.c_uint64(0)
    src = _p(buf, _u8p) if buf.size else C.cast(C.c_char_p(b""), _u8p)
    ptr = lib.alice_codec_encode_wide(encoder._h, src, buf.size, width, height, frames, lane_symbols, C.byref(n))
    if not ptr:
        _raise_last()
    try:
        return _copy_out(ptr, n.value).tobytes()
    finally:
        lib.alice_codec_data_free64(ptr, n.value)


def decode_wide(data) -> np.ndarray:
    """The RGB bytes of a version 3 container."""
    lib = load_library()
    buf = _as_u8(data)
    n = C.c_uint64(0)
    ptr = lib.alice_codec_decode_wide(_p(buf, _u8p), buf.size, C.byref(n))
    if not ptr:
        _raise_last()
    return _adopt(ptr, n.value, lib.alice_codec_data_free64)


def wide_stream_bound(n: int, lane_symbols: int = SPLIT_DEFAULT_LANE_SYMBOLS) -> int:
    return int(load_library().alice_codec_wide_stream_bound(n, lane_symbols))


def wide_encode_device(d_rgb_ptr: int, width: int, height: int, frames: int, n_chunks: int, wavelet_type: WaveletType,
                       quality: int, d_out_ptr: int, out_stride: int, qualities=None, lane_symbols: int = 0,
                       stream: int = 0) -> np.ndarray:
    """n_chunks packed device chunks -> version 3 bytes at d_out_ptr + i * out_stride; returns the sizes."""
    sizes = np.zeros(n_chunks, np.uint64)
    q = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8).reshape(-1)
    if q is not None and q.size != n_chunks:
        raise ValueError("one quality per chunk")
    _dims_u32(width, height, frames, n_chunks, lane_symbols)
    _check(load_library().alice_codec_dev_encode_wide(d_rgb_ptr, width, height, frames, n_chunks, int(wavelet_type), quality,
                                                      None if q is None else _p(q, _u8p), lane_symbols, d_out_ptr, out_stride,
                                                      _p(sizes, _u64p), stream or None))
    return sizes


def wide_decode_device(d_alc_ptr: int, alc_stride: int, sizes, d_rgb_out_ptr: int, stream: int = 0) -> None:
    s = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    _check(load_library().alice_codec_dev_decode_wide(d_alc_ptr, alc_stride, _p(s, _u64p), s.size, d_rgb_out_ptr, stream or None))


def forward_symbols_wide_device(d_rgb_ptr: int, width: int, height: int, frames: int, wavelet_type: WaveletType, quality: int,
                                d_symbols_ptr: int, d_hist_ptr: int = 0, stream: int = 0) -> None:
    """The 3 * padded u16 symbols encode_wide codes (Y, Co, Cg), and optionally the 3 x 256 histogram of min(z, 255)."""
    _dims_u32(width, height, frames)
    _check(load_library().alice_codec_dev_forward_symbols_wide(d_rgb_ptr, width, height, frames, int(wavelet_type), quality,
                                                               d_symbols_ptr, d_hist_ptr or None, stream or None))


def decode_alc(data) -> np.ndarray:
    """The RGB bytes of a container of any version: 1 (FrameDecoder), 2 (decode_split), 3 (decode_wide),
    4 (decode_reversible) or 5 (decode_banded)."""
    version = alc_version(data)
    if version == 2:
        return decode_split(data)
    if version == 3:
        return decode_wide(data)
    if version == 4:
        return decode_reversible(data)
    if version == 5:
        return decode_banded(data)
    return FrameDecoder().decode(EncodedChunk.from_bytes(data))   # version 1, and every refusal the v1 parser words


# ---- versions 2 and 3: size prediction, byte budgets, regions of device frames (DESIGN.md sections 10.8, 11.6) ----
# One body per call with the container as an argument, as in the library: `kind` is "split" (version 2) or "wide"
# (version 3) and names the C entry point.

def _predict_container_sizes(kind: str, rgb_frames, width: int, height: int, frames: int, wavelet_type, lane_symbols: int):
    r = _as_u8(rgb_frames)
    _dims_u32(width, height, frames, lane_symbols)
    lo = np.zeros(101, np.uint64); hi = np.zeros(101, np.uint64)
    ptr = _p(r, _u8p) if r.size else C.cast(C.c_char_p(b""), _u8p)
    fn = getattr(load_library(), f"alice_codec_predict_{kind}_sizes")
    _check(fn(int(wavelet_type), ptr, r.size, width, height, frames, lane_symbols, _p(lo, _u64p), _p(hi, _u64p)))
    return SizePrediction(lo, hi, np.zeros(101, np.uint8))


def _encode_container_to_size(kind: str, rgb_frames, width: int, height: int, frames: int, max_bytes: int, wavelet_type,
                              min_quality: int, max_quality: int, lane_symbols: int) -> tuple:
    lib = load_library()
    r = _as_u8(rgb_frames)
    _dims_u32(width, height, frames, lane_symbols)
    _check_budget_args([max_bytes], min_quality, max_quality)
    chosen = C.c_uint8(0); fits = C.c_uint8(0); n = C.c_uint64(0)
    src = _p(r, _u8p) if r.size else C.cast(C.c_char_p(b""), _u8p)
    ptr = getattr(lib, f"alice_codec_encode_{kind}_to_size")(int(wavelet_type), src, r.size, width, height, frames, lane_symbols,
                                                             int(max_bytes), int(min_quality), int(max_quality), C.byref(chosen),
                                                             C.byref(fits), C.byref(n))
    if not ptr:
        _raise_last()
    try:
        return _copy_out(ptr, n.value).tobytes(), int(chosen.value), bool(fits.value)
    finally:
        lib.alice_codec_data_free64(ptr, n.value)


def _origins_u32(origins, n_chunks: int) -> np.ndarray:
    o = np.ascontiguousarray(origins, dtype=np.int64).reshape(-1)
    if o.size != 2 * n_chunks or (o < 0).any() or (o > 0xFFFFFFFF).any():
        raise ValueError("origins: one (x, y) pair of u32 per chunk")
    return o.astype(np.uint32)


def _encode_container_regions(kind: str, d_frames_ptr: int, frame_width: int, frame_height: int, origins, width: int, height: int,
                              frames: int, wavelet_type, quality: int, d_out_ptr: int, out_stride: int, qualities,
                              lane_symbols: int, stream: int) -> np.ndarray:
    n_chunks = len(origins)
    o = _origins_u32(origins, n_chunks)
    sizes = np.zeros(n_chunks, np.uint64)
    q = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8).reshape(-1)
    if q is not None and q.size != n_chunks:
        raise ValueError("one quality per chunk")
    _dims_u32(frame_width, frame_height, width, height, frames, lane_symbols)
    fn = getattr(load_library(), f"alice_codec_dev_encode_{kind}_regions")
    _check(fn(d_frames_ptr, frame_width, frame_height, _p(o, _u32p), width, height, frames, n_chunks, int(wavelet_type), quality,
              None if q is None else _p(q, _u8p), lane_symbols, d_out_ptr, out_stride, _p(sizes, _u64p), stream or None))
    return sizes


def _decode_container_regions(kind: str, d_alc_ptr: int, alc_stride: int, sizes, d_frames_out_ptr: int, frame_width: int,
                              frame_height: int, origins, stream: int) -> None:
    s = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    o = _origins_u32(origins, s.size)
    _dims_u32(frame_width, frame_height)
    fn = getattr(load_library(), f"alice_codec_dev_decode_{kind}_regions")
    _check(fn(d_alc_ptr, alc_stride, _p(s, _u64p), s.size, d_frames_out_ptr, frame_width, frame_height, _p(o, _u32p), stream or None))


def _encode_container_to_budget(kind: str, d_frames_ptr: int, width: int, height: int, frames: int, n_chunks: int, wavelet_type,
                                budgets, d_out_ptr: int, out_stride: int, min_quality: int, max_quality: int, lane_symbols: int,
                                frame_width: int, frame_height: int, origins, stream: int) -> tuple:
    b = [int(v) for v in budgets]
    if len(b) != n_chunks:
        raise ValueError("one budget per chunk")
    _check_budget_args(b, min_quality, max_quality)
    _dims_u32(width, height, frames, n_chunks, lane_symbols, frame_width, frame_height)
    bud = np.array(b, dtype=np.uint64)
    o = None if origins is None else _origins_u32(origins, n_chunks)
    chosen = np.zeros(n_chunks, np.uint8); fits = np.zeros(n_chunks, np.uint8); sizes = np.zeros(n_chunks, np.uint64)
    fn = getattr(load_library(), f"alice_codec_dev_encode_{kind}_to_budget")
    _check(fn(d_frames_ptr, frame_width, frame_height, None if o is None else _p(o, _u32p), width, height, frames, n_chunks,
              int(wavelet_type), lane_symbols, _p(bud, _u64p), int(min_quality), int(max_quality), _p(chosen, _u8p), _p(fits, _u8p),
              d_out_ptr, out_stride, _p(sizes, _u64p), stream or None))
    return chosen, fits.astype(bool), sizes


# ---- version 2 ----

def predict_split_sizes(rgb_frames, width: int, height: int, frames: int, wavelet_type: WaveletType = WaveletType.Cdf53,
                        lane_symbols: int = 0) -> SizePrediction:
    """The size bracket of encode_split at every quality, from one forward transform on the GPU (no entropy coding).
    Every version 2 table is bounded: status is RATE_BOUNDED throughout."""
    return _predict_container_sizes("split", rgb_frames, width, height, frames, wavelet_type, lane_symbols)


def predict_split_sizes_device(d_rgb_ptr: int, width: int, height: int, frames: int, n_chunks: int,
                               wavelet_type: WaveletType = WaveletType.Cdf53, lane_symbols: int = 0,
                               stream: int = 0) -> SizePrediction:
    """n_chunks packed chunks at a device pointer: arrays of shape (n_chunks, 101)."""
    _dims_u32(width, height, frames, n_chunks, lane_symbols)
    lo = np.zeros((max(n_chunks, 1), 101), np.uint64); hi = np.zeros_like(lo)
    _check(load_library().alice_codec_dev_predict_split_sizes(d_rgb_ptr, width, height, frames, n_chunks, int(wavelet_type),
                                                              lane_symbols, _p(lo, _u64p), _p(hi, _u64p), stream or None))
    return SizePrediction(lo[:n_chunks], hi[:n_chunks], np.zeros((n_chunks, 101), np.uint8))


def encode_split_to_size(rgb_frames, width: int, height: int, frames: int, max_bytes: int,
                         wavelet_type: WaveletType = WaveletType.Cdf53, min_quality: int = 10, max_quality: int = 95,
                         lane_symbols: int = 0) -> tuple:
    """One chunk as version 2 bytes at the highest quality in [min_quality, max_quality] that fits max_bytes: the largest
    whose predicted upper bound fits, refined by at most four exact size counts among the qualities whose bracket straddles
    the budget.  Returns (bytes, quality, fits); fits is False when not even min_quality is guaranteed to fit (the chunk is
    then encoded at min_quality).  The bytes are encode_split's at that quality."""
    return _encode_container_to_size("split", rgb_frames, width, height, frames, max_bytes, wavelet_type, min_quality, max_quality,
                                     lane_symbols)


def split_encode_regions_device(d_frames_ptr: int, frame_width: int, frame_height: int, origins, width: int, height: int,
                                frames: int, wavelet_type: WaveletType, quality: int, d_out_ptr: int, out_stride: int,
                                qualities=None, lane_symbols: int = 0, stream: int = 0) -> np.ndarray:
    """Chunk i = frames [i * frames, (i + 1) * frames) of the device frames, cropped to width x height at origins[i], as
    version 2 bytes at d_out_ptr + i * out_stride (the bytes of encode_split of the crop); returns the sizes."""
    return _encode_container_regions("split", d_frames_ptr, frame_width, frame_height, origins, width, height, frames, wavelet_type,
                                     quality, d_out_ptr, out_stride, qualities, lane_symbols, stream)


def split_decode_regions_device(d_alc_ptr: int, alc_stride: int, sizes, d_frames_out_ptr: int, frame_width: int,
                                frame_height: int, origins, stream: int = 0) -> None:
    """Chunk i (sizes[i] bytes at d_alc_ptr + i * alc_stride) is decoded into its rectangle at origins[i] of its frames of
    d_frames_out_ptr; no byte outside the rectangles is written."""
    _decode_container_regions("split", d_alc_ptr, alc_stride, sizes, d_frames_out_ptr, frame_width, frame_height, origins, stream)


def split_encode_to_budget_device(d_frames_ptr: int, width: int, height: int, frames: int, n_chunks: int,
                                  wavelet_type: WaveletType, budgets, d_out_ptr: int, out_stride: int, min_quality: int = 10,
                                  max_quality: int = 95, lane_symbols: int = 0, frame_width: int = 0, frame_height: int = 0,
                                  origins=None, stream: int = 0) -> tuple:
    """n_chunks device chunks (packed, or regions of frame_width x frame_height frames when origins is given), chunk i at
    the quality encode_split_to_size's rule picks for budgets[i].  Returns (chosen, fits, sizes)."""
    return _encode_container_to_budget("split", d_frames_ptr, width, height, frames, n_chunks, wavelet_type, budgets, d_out_ptr,
                                       out_stride, min_quality, max_quality, lane_symbols, frame_width, frame_height, origins, stream)


# ---- version 3: the same calls for the wide container; lane_symbols is a power of two in
# [64, 8192], and a trial of the budget rule is the wide forward pass, the table and the wide count pass ----

def predict_wide_sizes(rgb_frames, width: int, height: int, frames: int, wavelet_type: WaveletType = WaveletType.Cdf53,
                       lane_symbols: int = 0) -> SizePrediction:
    """The size bracket of encode_wide at every quality, from one forward transform on the GPU (no entropy coding): the
    histogram of the coded symbol min(z, 255) at every step, with the 12-bit residual of every escape priced in.  Every
    version 3 table is bounded: status is RATE_BOUNDED throughout."""
    return _predict_container_sizes("wide", rgb_frames, width, height, frames, wavelet_type, lane_symbols)


def predict_wide_sizes_device(d_rgb_ptr: int, width: int, height: int, frames: int, n_chunks: int,
                              wavelet_type: WaveletType = WaveletType.Cdf53, lane_symbols: int = 0,
                              d_step_hist: int = 0, stream: int = 0) -> SizePrediction:
    """n_chunks packed chunks at a device pointer: arrays of shape (n_chunks, 101).  d_step_hist: 0, or a device pointer to
    n_chunks * 64 * 3 * 256 u32 that receives the histograms of the coded symbol min(z, 255) behind the prediction,
    [chunk][step - 1][channel][symbol]."""
    _dims_u32(width, height, frames, n_chunks, lane_symbols)
    lo = np.zeros((max(n_chunks, 1), 101), np.uint64); hi = np.zeros_like(lo)
    _check(load_library().alice_codec_dev_predict_wide_sizes(d_rgb_ptr, width, height, frames, n_chunks, int(wavelet_type),
                                                             lane_symbols, _p(lo, _u64p), _p(hi, _u64p), d_step_hist or None,
                                                             stream or None))
    return SizePrediction(lo[:n_chunks], hi[:n_chunks], np.zeros((n_chunks, 101), np.uint8))


def encode_wide_to_size(rgb_frames, width: int, height: int, frames: int, max_bytes: int,
                        wavelet_type: WaveletType = WaveletType.Cdf53, min_quality: int = 10, max_quality: int = 95,
                        lane_symbols: int = 0) -> tuple:
    """encode_split_to_size for version 3 (pass max_quality=100 for the top of the scale, where this container is the one
    to use).  Returns (bytes, quality, fits); the bytes are encode_wide's at that quality."""
    return _encode_container_to_size("wide", rgb_frames, width, height, frames, max_bytes, wavelet_type, min_quality, max_quality,
                                     lane_symbols)


def wide_encode_regions_device(d_frames_ptr: int, frame_width: int, frame_height: int, origins, width: int, height: int,
                               frames: int, wavelet_type: WaveletType, quality: int, d_out_ptr: int, out_stride: int,
                               qualities=None, lane_symbols: int = 0, stream: int = 0) -> np.ndarray:
    """split_encode_regions_device for version 3: the bytes of chunk i are encode_wide's of the crop; returns the sizes."""
    return _encode_container_regions("wide", d_frames_ptr, frame_width, frame_height, origins, width, height, frames, wavelet_type,
                                     quality, d_out_ptr, out_stride, qualities, lane_symbols, stream)


def wide_decode_regions_device(d_alc_ptr: int, alc_stride: int, sizes, d_frames_out_ptr: int, frame_width: int,
                               frame_height: int, origins, stream: int = 0) -> None:
    """split_decode_regions_device for version 3 containers: no byte outside the rectangles is written."""
    _decode_container_regions("wide", d_alc_ptr, alc_stride, sizes, d_frames_out_ptr, frame_width, frame_height, origins, stream)


def wide_encode_to_budget_device(d_frames_ptr: int, width: int, height: int, frames: int, n_chunks: int,
                                 wavelet_type: WaveletType, budgets, d_out_ptr: int, out_stride: int, min_quality: int = 10,
                                 max_quality: int = 95, lane_symbols: int = 0, frame_width: int = 0, frame_height: int = 0,
                                 origins=None, stream: int = 0) -> tuple:
    """split_encode_to_budget_device for version 3: chunk i at the quality encode_wide_to_size's rule picks for budgets[i].
    Returns (chosen, fits, sizes)."""
    return _encode_container_to_budget("wide", d_frames_ptr, width, height, frames, n_chunks, wavelet_type, budgets, d_out_ptr,
                                       out_stride, min_quality, max_quality, lane_symbols, frame_width, frame_height, origins, stream)


# ---- reversible format (.alc version 4) ----
# Version 3 whose decoder runs the forward lifting's mirror: at quality 100 (quantiser step 1) the pixels come back exactly.
# The container for lossless archival and intermediate storage; below quality 100 prefer version 3 (or 2).  The encoder is
# version 3's -- the bytes differ from encode_wide's in byte 4 only -- so predict_wide_sizes brackets a version 4 length
# exactly as it does a version 3 one and wide_stream_bound is the stream bound; there are no byte-budget calls.

LOSSLESS_QUALITY = 100


def reversible_info(data) -> SplitInfo:
    """The header fields of a version 4 container (validated, no device needed); the fields are version 2's."""
    buf = _as_u8(data)
    c = _CSplitInfo()
    _check(load_library().alice_codec_reversible_info(_p(buf, _u8p), buf.size, C.byref(c)))
    return SplitInfo(c)


def encode_reversible(encoder: "FrameEncoder", rgb_frames, width: int, height: int, frames: int, lane_symbols: int = 0) -> bytes:
    """One chunk as version 4 bytes, with the encoder's wavelet and quality (lane_symbols 0: the default)."""
    lib = load_library()
    buf = _as_u8(rgb_frames)
    _dims_u32(width, height, frames, lane_symbols)
    n = C.c_uint64(0)
    src = _p(buf, _u8p) if buf.size else C.cast(C.c_char_p(b""), _u8p)
    ptr = lib.alice_codec_encode_reversible(encoder._h, src, buf.size, width, height, frames, lane_symbols, C.byref(n))
    if not ptr:
        _raise_last()
    try:
        return _copy_out(ptr, n.value).tobytes()
    finally:
        lib.alice_codec_data_free64(ptr, n.value)


def decode_reversible(data) -> np.ndarray:
    """The RGB bytes of a version 4 container."""
    lib = load_library()
    buf = _as_u8(data)
    n = C.c_uint64(0)
    ptr = lib.alice_codec_decode_reversible(_p(buf, _u8p), buf.size, C.byref(n))
    if not ptr:
        _raise_last()
    return _adopt(ptr, n.value, lib.alice_codec_data_free64)


def encode_lossless(rgb_frames, width: int, height: int, frames: int, wavelet_type: WaveletType = WaveletType.Cdf53,
                    lane_symbols: int = 0) -> bytes:
    """One chunk as version 4 bytes at quality 100: decode_reversible (or decode_alc) returns rgb_frames exactly."""
    return encode_reversible(FrameEncoder(LOSSLESS_QUALITY, WaveletType(wavelet_type)), rgb_frames, width, height, frames, lane_symbols)


def reversible_encode_device(d_rgb_ptr: int, width: int, height: int, frames: int, n_chunks: int, wavelet_type: WaveletType,
                             quality: int, d_out_ptr: int, out_stride: int, qualities=None, lane_symbols: int = 0,
                             stream: int = 0) -> np.ndarray:
    """n_chunks packed device chunks -> version 4 bytes at d_out_ptr + i * out_stride; returns the sizes."""
    sizes = np.zeros(n_chunks, np.uint64)
    q = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8).reshape(-1)
    if q is not None and q.size != n_chunks:
        raise ValueError("one quality per chunk")
    _dims_u32(width, height, frames, n_chunks, lane_symbols)
    _check(load_library().alice_codec_dev_encode_reversible(d_rgb_ptr, width, height, frames, n_chunks, int(wavelet_type), quality,
                                                            None if q is None else _p(q, _u8p), lane_symbols, d_out_ptr,
                                                            out_stride, _p(sizes, _u64p), stream or None))
    return sizes


def encode_lossless_device(d_rgb_ptr: int, width: int, height: int, frames: int, n_chunks: int, d_out_ptr: int, out_stride: int,
                           wavelet_type: WaveletType = WaveletType.Cdf53, lane_symbols: int = 0, stream: int = 0) -> np.ndarray:
    """reversible_encode_device at quality 100 for every chunk; returns the sizes."""
    return reversible_encode_device(d_rgb_ptr, width, height, frames, n_chunks, wavelet_type, LOSSLESS_QUALITY, d_out_ptr, out_stride,
                                    lane_symbols=lane_symbols, stream=stream)


def reversible_decode_device(d_alc_ptr: int, alc_stride: int, sizes, d_rgb_out_ptr: int, stream: int = 0) -> None:
    s = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    _check(load_library().alice_codec_dev_decode_reversible(d_alc_ptr, alc_stride, _p(s, _u64p), s.size, d_rgb_out_ptr,
                                                            stream or None))


def reversible_encode_regions_device(d_frames_ptr: int, frame_width: int, frame_height: int, origins, width: int, height: int,
                                     frames: int, wavelet_type: WaveletType, quality: int, d_out_ptr: int, out_stride: int,
                                     qualities=None, lane_symbols: int = 0, stream: int = 0) -> np.ndarray:
    """wide_encode_regions_device for version 4: the bytes of chunk i are encode_reversible's of the crop; returns the sizes."""
    return _encode_container_regions("reversible", d_frames_ptr, frame_width, frame_height, origins, width, height, frames,
                                     wavelet_type, quality, d_out_ptr, out_stride, qualities, lane_symbols, stream)


def reversible_decode_regions_device(d_alc_ptr: int, alc_stride: int, sizes, d_frames_out_ptr: int, frame_width: int,
                                     frame_height: int, origins, stream: int = 0) -> None:
    """wide_decode_regions_device for version 4: no byte outside the rectangles is written."""
    _decode_container_regions("reversible", d_alc_ptr, alc_stride, sizes, d_frames_out_ptr, frame_width, frame_height, origins,
                              stream)


# ---- frame ranges of a version 2, 3 or 4 chunk ----

def frames_window(wavelet_type: WaveletType, frames: int, first: int, count: int) -> tuple:
    """(a, b): frames [first, first + count) of a chunk of `frames` frames depend on the coefficient planes of the frame
    pairs inside [a, b) only.  No device needed."""
    _dims_u32(frames, first, count)
    a, b = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().alice_codec_frames_window(int(wavelet_type), frames, first, count, C.byref(a), C.byref(b)))
    return a.value, b.value


def decode_frames(data, first: int, count: int) -> np.ndarray:
    """The RGB bytes of frames [first, first + count) of a version 2, 3 or 4 container, from the blocks they need: only the
    header, the block-length tables and those blocks are read and uploaded (data may be an np.memmap).  The end checks
    cover the blocks that are read."""
    lib = load_library()
    buf = _as_u8(data)
    _dims_u32(first, count)
    n = C.c_uint64(0)
    ptr = lib.alice_codec_decode_frames(_p(buf, _u8p), buf.size, first, count, C.byref(n))
    if not ptr:
        _raise_last()
    return _adopt(ptr, n.value, lib.alice_codec_data_free64)


def frames_decode_device(d_alc_ptr: int, length: int, first: int, count: int, d_rgb_out_ptr: int, stream: int = 0) -> None:
    """decode_frames of a device-resident container of `length` bytes into count packed frames at d_rgb_out_ptr."""
    _dims_u32(first, count)
    _check(load_library().alice_codec_dev_decode_frames(d_alc_ptr, length, first, count, d_rgb_out_ptr, stream or None))


def _test_last_frames_stats() -> tuple:
    """(a, b, blocks decoded over the three channels, payload bytes the host call uploaded, frames of the spatial pass) of
    the calling thread's last frame-range decode."""
    out = np.zeros(5, np.uint64)
    load_library().alice_codec_test_last_frames_stats(_p(out, _u64p))
    return tuple(int(v) for v in out)


# ---- half-resolution preview of a version 2, 3 or 4 chunk from the low band alone ----

def preview_dims(width: int, height: int) -> tuple:
    """(qw, qh) = (ceil(width / 2), ceil(height / 2)): the size of a preview frame.  No device needed."""
    _dims_u32(width, height)
    qw, qh = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().alice_codec_preview_dims(width, height, C.byref(qw), C.byref(qh)))
    return qw.value, qh.value


def decode_preview(data, first: int, count: int) -> np.ndarray:
    """The half-resolution RGB bytes (count * qh * qw * 3) of frames [first, first + count) of a version 2, 3 or 4 container,
    from the low-low quadrants of the coefficient planes the range needs: only the header, the block-length tables and the
    blocks of the planes' top halves are read and uploaded (data may be an np.memmap), and no spatial inverse runs.  The end
    checks cover the blocks that are read."""
    lib = load_library()
    buf = _as_u8(data)
    _dims_u32(first, count)
    n = C.c_uint64(0)
    ptr = lib.alice_codec_decode_preview(_p(buf, _u8p), buf.size, first, count, C.byref(n))
    if not ptr:
        _raise_last()
    return _adopt(ptr, n.value, lib.alice_codec_data_free64)


def preview_decode_device(d_alc_ptr: int, length: int, first: int, count: int, d_rgb_out_ptr: int, stream: int = 0) -> None:
    """decode_preview of a device-resident container of `length` bytes into count packed preview frames at d_rgb_out_ptr."""
    _dims_u32(first, count)
    _check(load_library().alice_codec_dev_decode_preview(d_alc_ptr, length, first, count, d_rgb_out_ptr, stream or None))


def _test_last_preview_stats() -> tuple:
    """(a, b, blocks decoded over the three channels, payload bytes the host call uploaded, frames written, symbols stored
    over the three channels) of the calling thread's last preview decode."""
    out = np.zeros(6, np.uint64)
    load_library().alice_codec_test_last_preview_stats(_p(out, _u64p))
    return tuple(int(v) for v in out)


# ---- many previews in one call ----

def _previews_error(bad: int):
    """Raises the library's last error with the index of the item that decided it (None: no item's) as .bad_item"""
    try:
        _raise_last()
    except CodecError as e:
        e.bad_item = None if bad == PREVIEWS_NO_ITEM else bad
        raise


def _preview_items(rows):
    n = len(rows)
    if n > 0xFFFFFFFF:
        raise CodecError(3, "dimension out of u32 range")
    arr = (PreviewItem * max(n, 1))()
    for i, (alc, length, first, count, out) in enumerate(rows):
        _dims_u32(first, count)
        arr[i] = PreviewItem(alc, length, first, count, out)
    return arr


def decode_previews(items) -> list:
    """decode_preview of many (data, first, count) items in one call: a list of arrays, one per item, in item order.  Items
    may mix versions 2, 3 and 4, wavelets, sizes and lane sizes; items that pass the same object as data share its header,
    tables, directory scan and upload (the union of their planned blocks goes up once).  All or nothing: the first item that
    is refused or damaged decides the CodecError, whose .bad_item is its index and whose message starts with "item <index>"."""
    lib = load_library()
    items = list(items)
    bufs, rows = {}, []
    for data, first, count in items:
        buf = bufs.setdefault(id(data), _as_u8(data))
        rows.append((buf.ctypes.data, buf.size, first, count, None))
    arr = _preview_items(rows)
    offsets = np.zeros(len(rows) + 1, np.uint64)
    bad = C.c_uint32(PREVIEWS_NO_ITEM)
    ptr = lib.alice_codec_decode_previews(arr, len(rows), _p(offsets, _u64p), C.byref(bad))
    if not ptr:
        _previews_error(bad.value)
    whole = _adopt(ptr, int(offsets[-1]), lib.alice_codec_data_free64)
    return [whole[int(offsets[i]):int(offsets[i + 1])] for i in range(len(rows))]


def previews_decode_device(items, stream: int = 0) -> None:
    """preview_decode_device of many (d_alc_ptr, length, first, count, d_rgb_out_ptr) items in one call (containers and
    outputs on the device; outputs must not overlap).  Items that name the same pointer and length share their header,
    tables and directory scan.  All or nothing, errors as decode_previews."""
    rows = [tuple(r) for r in items]
    arr = _preview_items(rows)
    bad = C.c_uint32(PREVIEWS_NO_ITEM)
    if load_library().alice_codec_dev_decode_previews(arr, len(rows), C.byref(bad), stream or None) != 0:
        _previews_error(bad.value)


def _test_last_previews_stats() -> tuple:
    """(items, distinct containers, table launches, lane launches, finish launches, stream drains, blocks decoded, payload
    bytes the host call uploaded, symbols stored) of the calling thread's last batched preview that ran to its end."""
    out = np.zeros(9, np.uint64)
    load_library().alice_codec_test_last_previews_stats(_p(out, _u64p))
    return tuple(int(v) for v in out)


# ---- a spatial rectangle of a frame range of a version 2, 3 or 4 chunk ----

def rect_window(wavelet_type: WaveletType, width: int, height: int, x: int, y: int, w: int, h: int) -> tuple:
    """(xa, xb, ya, yb): the w x h pixels at (x, y) of a width x height frame depend on the coefficient columns inside
    [xa, xb) and rows inside [ya, yb) only.  No device needed."""
    _dims_u32(width, height, x, y, w, h)
    v = [C.c_uint32(0) for _ in range(4)]
    _check(load_library().alice_codec_rect_window(int(wavelet_type), width, height, x, y, w, h, *[C.byref(c) for c in v]))
    return tuple(c.value for c in v)


def decode_rect(data, first: int, count: int, x: int, y: int, w: int, h: int) -> np.ndarray:
    """The RGB bytes (count * h * w * 3, packed) of the w x h rectangle at (x, y) of frames [first, first + count) of a
    version 2, 3 or 4 container, from the blocks they need: only the header, the block-length tables and those blocks are
    read and uploaded (data may be an np.memmap).  The end checks cover the blocks that are read."""
    lib = load_library()
    buf = _as_u8(data)
    _dims_u32(first, count, x, y, w, h)
    n = C.c_uint64(0)
    ptr = lib.alice_codec_decode_rect(_p(buf, _u8p), buf.size, first, count, x, y, w, h, C.byref(n))
    if not ptr:
        _raise_last()
    return _adopt(ptr, n.value, lib.alice_codec_data_free64)


def rect_decode_device(d_alc_ptr: int, length: int, first: int, count: int, x: int, y: int, w: int, h: int, d_rgb_out_ptr: int,
                       row_pitch: int = 0, frame_pitch: int = 0, stream: int = 0) -> None:
    """decode_rect of a device-resident container of `length` bytes to d_rgb_out_ptr: packed when both pitches are 0, else
    row r of frame k at k * frame_pitch + r * row_pitch (bytes), so that the rectangle can be pasted into full-size frames.
    Only the 3 w bytes of each of the h rows of each frame are written."""
    _dims_u32(first, count, x, y, w, h)
    _check(load_library().alice_codec_dev_decode_rect(d_alc_ptr, length, first, count, x, y, w, h, d_rgb_out_ptr, row_pitch, frame_pitch,
                                                      stream or None))


def _test_last_rect_stats() -> tuple:
    """(ta, tb, xa, xb, ya, yb, blocks decoded over the three channels, payload bytes the host call uploaded, frames
    written, symbols stored over the three channels) of the calling thread's last rectangle decode."""
    out = np.zeros(10, np.uint64)
    load_library().alice_codec_test_last_rect_stats(_p(out, _u64p))
    return tuple(int(v) for v in out)


# ---- many frame ranges and rectangles in one call ----

def _rect_items(rows):
    n = len(rows)
    if n > 0xFFFFFFFF:
        raise CodecError(3, "dimension out of u32 range")
    arr = (RectItem * max(n, 1))()
    for i, (alc, length, first, count, x, y, w, h, out, row_pitch, frame_pitch) in enumerate(rows):
        _dims_u32(first, count, x, y, w, h)
        arr[i] = RectItem(alc, length, first, count, x, y, w, h, out, row_pitch, frame_pitch)
    return arr


def decode_rects(items) -> list:
    """decode_frames / decode_rect of many items in one call: (data, first, count) is the whole frames, (data, first, count,
    x, y, w, h) the w x h rectangle at (x, y).  A list of arrays, one per item (count * h * w * 3 packed bytes), in item
    order.  Items may mix versions 2, 3 and 4, wavelets, sizes, lane sizes, ranges and rectangles; items that pass the same
    object as data share its header, tables, directory scan and upload (the union of their planned blocks goes up once).
    All or nothing: the first item that is refused or damaged decides the CodecError, whose .bad_item is its index and whose
    message starts with "item <index>"."""
    lib = load_library()
    bufs, rows = {}, []
    for item in list(items):
        data, first, count = item[:3]
        x, y, w, h = item[3:] if len(item) > 3 else (0, 0, 0, 0)
        buf = bufs.setdefault(id(data), _as_u8(data))
        rows.append((buf.ctypes.data, buf.size, first, count, x, y, w, h, None, 0, 0))
    arr = _rect_items(rows)
    offsets = np.zeros(len(rows) + 1, np.uint64)
    bad = C.c_uint32(PREVIEWS_NO_ITEM)
    ptr = lib.alice_codec_decode_rects(arr, len(rows), _p(offsets, _u64p), C.byref(bad))
    if not ptr:
        _previews_error(bad.value)
    whole = _adopt(ptr, int(offsets[-1]), lib.alice_codec_data_free64)
    return [whole[int(offsets[i]):int(offsets[i + 1])] for i in range(len(rows))]


def rects_decode_device(items, stream: int = 0) -> None:
    """rect_decode_device of many (d_alc_ptr, length, first, count, x, y, w, h, d_rgb_out_ptr, row_pitch, frame_pitch) items
    in one call (containers and outputs on the device; x = y = w = h = 0 is the whole frame).  Outputs must be disjoint:
    byte ranges that do not intersect, or boxes of one pitched surface that do not (a mosaic).  Items that name the same
    pointer and length share their header, tables and directory scan.  All or nothing, errors as decode_rects."""
    rows = [tuple(r) for r in items]
    arr = _rect_items(rows)
    bad = C.c_uint32(PREVIEWS_NO_ITEM)
    if load_library().alice_codec_dev_decode_rects(arr, len(rows), C.byref(bad), stream or None) != 0:
        _previews_error(bad.value)


def _test_last_rects_stats() -> tuple:
    """(items, distinct containers, table launches, lane launches, batched finish launches, items finished through the
    per-item path, stream drains, blocks decoded, payload bytes the host call uploaded, symbols stored, frames written) of
    the calling thread's last batched frame-range / rectangle decode that ran to its end."""
    out = np.zeros(11, np.uint64)
    load_library().alice_codec_test_last_rects_stats(_p(out, _u64p))
    return tuple(int(v) for v in out)


def _test_rects_outputs_disjoint(items):
    """The output-disjointness rule of rects_decode_device on (d_rgb_out_ptr, count, w, h, row_pitch, frame_pitch) rows; no
    device.  None when no two conflict, else the index of the later item of the first conflicting pair."""
    rows = [(1, 0, 0, count, 0, 0, w, h, out, rp, fp) for out, count, w, h, rp, fp in items]
    arr = _rect_items(rows)
    bad = C.c_uint32(PREVIEWS_NO_ITEM)
    if load_library().alice_codec_test_rects_outputs_disjoint(arr, len(rows), C.byref(bad)) != 0:
        return bad.value
    return None


# ---- quality control: exact trial distortion and PSNR-floor encodes ----

FORMAT_SPLIT, FORMAT_WIDE, FORMAT_REVERSIBLE = 2, 3, 4
QUALITY_MAX_TRIALS = 8
_FORMAT_BYTE = {"split": FORMAT_SPLIT, "wide": FORMAT_WIDE, "reversible": FORMAT_REVERSIBLE}


def _format_byte(format) -> int:
    """'split' / 'wide' / 'reversible' or the version byte itself (the library refuses the bytes it does not know)."""
    if isinstance(format, str):
        if format not in _FORMAT_BYTE:
            raise CodecError(4, f"format must be 'split', 'wide' or 'reversible', got {format!r}")
        return _FORMAT_BYTE[format]
    v = int(format)
    if not 0 <= v <= 255:
        raise CodecError(4, f"format byte must fit a u8, got {format}")
    return v


def _check_min_psnr(min_psnr) -> float:
    t = float(min_psnr)
    if t != t or t < 0.0:
        raise CodecError(2, "min_psnr must be a number >= 0 (or inf for exact)")
    return t


def psnr_from_sse(sse: int, n_bytes: int) -> float:
    """The dB value of a squared error over n_bytes samples, by the expression psnr() uses: inf at 0."""
    return float(load_library().alice_codec_psnr_from_sse(int(sse), int(n_bytes)))


def rgb_sse_device(d_a_ptr: int, d_b_ptr: int, width: int, height: int, n_frames: int, a_pitches=None, b_pitches=None,
                   d_frame_sse_ptr: int | None = None, stream: int = 0):
    """Exact squared error per frame of two device volumes of n_frames frames of width x height interleaved RGB.  A side's
    pitches are (row_pitch, frame_pitch) in bytes (None: packed); the pointers may have any byte alignment.  The n_frames
    u64 sums go to d_frame_sse_ptr when given (returns None), else they are returned as an array."""
    _dims_u32(width, height)
    packed = (3 * width, 3 * width * height)
    ap = tuple(int(v) for v in (a_pitches or packed)); bp = tuple(int(v) for v in (b_pitches or packed))
    fn = load_library().alice_codec_dev_rgb_sse
    if d_frame_sse_ptr is not None:
        _check(fn(d_a_ptr, ap[0], ap[1], d_b_ptr, bp[0], bp[1], width, height, int(n_frames), d_frame_sse_ptr, stream or None))
        return None
    import torch
    out = torch.empty(max(int(n_frames), 1), dtype=torch.int64, device="cuda")
    _check(fn(d_a_ptr, ap[0], ap[1], d_b_ptr, bp[0], bp[1], width, height, int(n_frames), out.data_ptr(), stream or None))
    return out.cpu().numpy().view(np.uint64)[:int(n_frames)]


def trial_sse_device(format, d_frames_ptr: int, width: int, height: int, frames: int, n_chunks: int, wavelet_type: WaveletType,
                     quality: int, qualities=None, frame_width: int = 0, frame_height: int = 0, origins=None,
                     d_frame_sse_ptr: int | None = None, stream: int = 0) -> np.ndarray:
    """The squared error, per chunk, between the source and what the format's decode returns for the format's encode at the
    given quality (chunk i at qualities[i] when given): a forward and an inverse transform and one comparison pass, no
    entropy coding.  Packed chunks, or regions of frame_width x frame_height frames when origins is given.
    d_frame_sse_ptr: device memory for n_chunks * frames u64 that receives the per-frame sums."""
    _dims_u32(width, height, frames, n_chunks, frame_width, frame_height)
    q = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8).reshape(-1)
    if q is not None and q.size != n_chunks:
        raise ValueError("one quality per chunk")
    o = None if origins is None else _origins_u32(origins, n_chunks)
    sse = np.zeros(max(n_chunks, 1), np.uint64)
    _check(load_library().alice_codec_dev_trial_sse(_format_byte(format), d_frames_ptr, frame_width, frame_height,
                                                    None if o is None else _p(o, _u32p), width, height, frames, n_chunks,
                                                    int(wavelet_type), int(quality), None if q is None else _p(q, _u8p),
                                                    _p(sse, _u64p), d_frame_sse_ptr, stream or None))
    return sse[:n_chunks]


def trial_psnr_device(format, d_frames_ptr: int, width: int, height: int, frames: int, n_chunks: int, wavelet_type: WaveletType,
                      quality: int, qualities=None, frame_width: int = 0, frame_height: int = 0, origins=None,
                      stream: int = 0) -> np.ndarray:
    """trial_sse_device as dB per chunk (psnr_from_sse over the chunk's width * height * frames * 3 samples)."""
    sse = trial_sse_device(format, d_frames_ptr, width, height, frames, n_chunks, wavelet_type, quality, qualities, frame_width,
                           frame_height, origins, None, stream)
    n = int(width) * int(height) * int(frames) * 3
    return np.array([psnr_from_sse(int(s), n) for s in sse], dtype=np.float64)


def _encode_container_to_psnr(kind: str, rgb_frames, width: int, height: int, frames: int, min_psnr, wavelet_type,
                              min_quality: int, max_quality: int, lane_symbols: int) -> tuple:
    lib = load_library()
    r = _as_u8(rgb_frames)
    _dims_u32(width, height, frames, lane_symbols)
    _check_budget_args([0], min_quality, max_quality)
    t = _check_min_psnr(min_psnr)
    chosen = C.c_uint8(0); reached = C.c_uint8(0); db = C.c_double(0.0); n = C.c_uint64(0)
    src = _p(r, _u8p) if r.size else C.cast(C.c_char_p(b""), _u8p)
    ptr = lib.alice_codec_encode_to_psnr(_format_byte(kind), int(wavelet_type), src, r.size, width, height, frames, lane_symbols, t,
                                         int(min_quality), int(max_quality), C.byref(chosen), C.byref(reached), C.byref(db),
                                         C.byref(n))
    if not ptr:
        _raise_last()
    try:
        return _copy_out(ptr, n.value).tobytes(), int(chosen.value), bool(reached.value), float(db.value)
    finally:
        lib.alice_codec_data_free64(ptr, n.value)


def _encode_container_to_psnr_device(kind: str, d_frames_ptr: int, width: int, height: int, frames: int, n_chunks: int, wavelet_type,
                                     min_psnr, d_out_ptr: int, out_stride: int, min_quality: int, max_quality: int,
                                     lane_symbols: int, frame_width: int, frame_height: int, origins, stream: int) -> tuple:
    _check_budget_args([0], min_quality, max_quality)
    t = _check_min_psnr(min_psnr)
    _dims_u32(width, height, frames, n_chunks, lane_symbols, frame_width, frame_height)
    o = None if origins is None else _origins_u32(origins, n_chunks)
    m = max(n_chunks, 1)
    chosen = np.zeros(m, np.uint8); reached = np.zeros(m, np.uint8); db = np.zeros(m, np.float64); sizes = np.zeros(m, np.uint64)
    _check(load_library().alice_codec_dev_encode_to_psnr(_format_byte(kind), d_frames_ptr, frame_width, frame_height,
                                                         None if o is None else _p(o, _u32p), width, height, frames, n_chunks,
                                                         int(wavelet_type), lane_symbols, t, int(min_quality), int(max_quality),
                                                         _p(chosen, _u8p), _p(reached, _u8p), _p(db, C.POINTER(C.c_double)),
                                                         d_out_ptr, out_stride, _p(sizes, _u64p), stream or None))
    return chosen[:n_chunks], reached[:n_chunks].astype(bool), db[:n_chunks], sizes[:n_chunks]


def encode_split_to_psnr(rgb_frames, width: int, height: int, frames: int, min_psnr: float,
                         wavelet_type: WaveletType = WaveletType.Cdf53, min_quality: int = 10, max_quality: int = 95,
                         lane_symbols: int = 0) -> tuple:
    """One chunk as version 2 bytes at the lowest quality in [min_quality, max_quality] whose measured PSNR is at least
    min_psnr dB: the finest and the coarsest quantiser step of the range are tried, then bisection, at most eight exact
    trials (a transform pair and a comparison each, no entropy coding).  Returns (bytes, quality, reached, psnr): reached is
    False when not even max_quality reaches the floor (the chunk is then encoded at max_quality), psnr is the measured value
    of the point returned.  The bytes are encode_split's at that quality.  Version 2 wraps at qualities 97 and above: keep
    max_quality <= 96 or use encode_wide_to_psnr."""
    return _encode_container_to_psnr("split", rgb_frames, width, height, frames, min_psnr, wavelet_type, min_quality, max_quality,
                                     lane_symbols)


def encode_wide_to_psnr(rgb_frames, width: int, height: int, frames: int, min_psnr: float,
                        wavelet_type: WaveletType = WaveletType.Cdf53, min_quality: int = 10, max_quality: int = 95,
                        lane_symbols: int = 0) -> tuple:
    """encode_split_to_psnr for version 3: the bytes are encode_wide's at the returned quality."""
    return _encode_container_to_psnr("wide", rgb_frames, width, height, frames, min_psnr, wavelet_type, min_quality, max_quality,
                                     lane_symbols)


def split_encode_to_psnr_device(d_frames_ptr: int, width: int, height: int, frames: int, n_chunks: int,
                                wavelet_type: WaveletType, min_psnr: float, d_out_ptr: int, out_stride: int, min_quality: int = 10,
                                max_quality: int = 95, lane_symbols: int = 0, frame_width: int = 0, frame_height: int = 0,
                                origins=None, stream: int = 0) -> tuple:
    """n_chunks device chunks (packed, or regions of frame_width x frame_height frames when origins is given), chunk i at
    the quality encode_split_to_psnr's rule picks for it.  Returns (chosen, reached, psnr, sizes)."""
    return _encode_container_to_psnr_device("split", d_frames_ptr, width, height, frames, n_chunks, wavelet_type, min_psnr, d_out_ptr,
                                            out_stride, min_quality, max_quality, lane_symbols, frame_width, frame_height, origins,
                                            stream)


def wide_encode_to_psnr_device(d_frames_ptr: int, width: int, height: int, frames: int, n_chunks: int,
                               wavelet_type: WaveletType, min_psnr: float, d_out_ptr: int, out_stride: int, min_quality: int = 10,
                               max_quality: int = 95, lane_symbols: int = 0, frame_width: int = 0, frame_height: int = 0,
                               origins=None, stream: int = 0) -> tuple:
    """split_encode_to_psnr_device for version 3."""
    return _encode_container_to_psnr_device("wide", d_frames_ptr, width, height, frames, n_chunks, wavelet_type, min_psnr, d_out_ptr,
                                            out_stride, min_quality, max_quality, lane_symbols, frame_width, frame_height, origins,
                                            stream)


# ---- transcode of a version 2, 3 or 4 chunk to a lower quality or a byte budget, without pixels ----

def _u8_arg(v, what: str) -> int:
    if not 0 <= int(v) <= 255:
        raise ValueError(f"{what} must fit a u8 (0..255), got {v}")
    return int(v)


def transcode(data, quality: int, lane_symbols: int = 0, out_version: int = 0) -> bytes:
    """A version 2, 3 or 4 container at `quality`, made from its symbols alone: lane decode, a map of every symbol to the
    coarser quantiser step, table, lane encode.  A channel whose step is already at or above the target's is left as it is,
    so a quality at or above the source's returns the source's bytes.  From a quality-100 source the result is byte for
    byte the direct encode at `quality`.  lane_symbols 0 keeps the source's; out_version 0 keeps the version (3 and 4 may be
    exchanged).  The result is read by the ordinary decode calls (decode_alc)."""
    lib = load_library()
    buf = _as_u8(data)
    _dims_u32(lane_symbols)
    n = C.c_uint64(0)
    ptr = lib.alice_codec_transcode(_p(buf, _u8p), buf.size, _u8_arg(quality, "quality"), lane_symbols, _u8_arg(out_version, "out_version"),
                                    C.byref(n))
    if not ptr:
        _raise_last()
    try:
        return _copy_out(ptr, n.value).tobytes()
    finally:
        lib.alice_codec_data_free64(ptr, n.value)


def transcode_to_size(data, max_bytes: int, min_quality: int = 10, max_quality: int = 95, lane_symbols: int = 0,
                      out_version: int = 0) -> tuple:
    """transcode at the highest quality in [min_quality, max_quality] that the byte-budget rule of encode_split_to_size finds
    to fit max_bytes (brackets from predict_transcode_sizes, at most four exact trials from the decoded symbols).  Returns
    (bytes, quality, fits); the bytes are transcode's at that quality.  A version 4 result has no budget: out_version=3."""
    lib = load_library()
    buf = _as_u8(data)
    _dims_u32(lane_symbols)
    _check_budget_args([max_bytes], min_quality, max_quality)
    chosen = C.c_uint8(0); fits = C.c_uint8(0); n = C.c_uint64(0)
    ptr = lib.alice_codec_transcode_to_size(_p(buf, _u8p), buf.size, lane_symbols, _u8_arg(out_version, "out_version"), int(max_bytes),
                                            int(min_quality), int(max_quality), C.byref(chosen), C.byref(fits), C.byref(n))
    if not ptr:
        _raise_last()
    try:
        return _copy_out(ptr, n.value).tobytes(), int(chosen.value), bool(fits.value)
    finally:
        lib.alice_codec_data_free64(ptr, n.value)


def predict_transcode_sizes(data, lane_symbols: int = 0) -> SizePrediction:
    """lo[q] <= len(transcode(data, q, lane_symbols)) <= hi[q] for the 101 qualities (status is always bounded)."""
    buf = _as_u8(data)
    _dims_u32(lane_symbols)
    lo = np.zeros(101, np.uint64); hi = np.zeros(101, np.uint64)
    _check(load_library().alice_codec_predict_transcode_sizes(_p(buf, _u8p), buf.size, lane_symbols, _p(lo, _u64p), _p(hi, _u64p)))
    return SizePrediction(lo, hi, np.zeros(101, np.uint8))


def transcode_device(d_alc_ptr: int, alc_stride: int, sizes, quality: int, d_out_ptr: int, out_stride: int, qualities=None,
                     lane_symbols: int = 0, out_version: int = 0, stream: int = 0) -> np.ndarray:
    """len(sizes) device containers of one version, wavelet, shape and lane_symbols (chunk i of sizes[i] bytes at
    d_alc_ptr + i * alc_stride) -> chunk i transcoded to qualities[i] (None: `quality`) at d_out_ptr + i * out_stride;
    returns the sizes."""
    s = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    q = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8).reshape(-1)
    if q is not None and q.size != s.size:
        raise ValueError("one quality per chunk")
    _dims_u32(lane_symbols)
    out = np.zeros(s.size, np.uint64)
    _check(load_library().alice_codec_dev_transcode(d_alc_ptr, alc_stride, _p(s, _u64p), s.size, _u8_arg(quality, "quality"),
                                                    None if q is None else _p(q, _u8p), lane_symbols, _u8_arg(out_version, "out_version"),
                                                    d_out_ptr, out_stride, _p(out, _u64p), stream or None))
    return out


def transcode_to_budget_device(d_alc_ptr: int, alc_stride: int, sizes, budgets, d_out_ptr: int, out_stride: int, min_quality: int = 10,
                               max_quality: int = 95, lane_symbols: int = 0, out_version: int = 0, stream: int = 0) -> tuple:
    """transcode_device with chunk i under budgets[i] bytes by transcode_to_size's rule.  Returns (chosen, fits, sizes)."""
    s = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    b = [int(v) for v in budgets]
    if len(b) != s.size:
        raise ValueError("one budget per chunk")
    _check_budget_args(b, min_quality, max_quality)
    _dims_u32(lane_symbols)
    bud = np.array(b, dtype=np.uint64)
    chosen = np.zeros(s.size, np.uint8); fits = np.zeros(s.size, np.uint8); out = np.zeros(s.size, np.uint64)
    _check(load_library().alice_codec_dev_transcode_to_budget(d_alc_ptr, alc_stride, _p(s, _u64p), s.size, lane_symbols,
                                                              _u8_arg(out_version, "out_version"), _p(bud, _u64p), int(min_quality),
                                                              int(max_quality), _p(chosen, _u8p), _p(fits, _u8p), d_out_ptr, out_stride,
                                                              _p(out, _u64p), stream or None))
    return chosen, fits.astype(bool), out


def requant_symbols_device(d_src_ptr: int, d_dst_ptr: int, n: int, wide: bool, step_from: int, step_to: int, d_hist_ptr: int = 0,
                           stream: int = 0) -> None:
    """Stage call: n device symbols (u8; wide: u16) from d_src_ptr to d_dst_ptr (the same address, or no overlap) through the
    transcode map of quantiser steps (step_from, step_to); the histogram of the coded symbols is added to the 256 u32 at
    d_hist_ptr when given."""
    if not 0 <= n < (1 << 64):
        raise CodecError(3, "symbol count out of u64 range")
    if not (-(1 << 31) <= step_from < (1 << 31) and -(1 << 31) <= step_to < (1 << 31)):
        raise CodecError(5, "quantiser step out of i32 range")
    _check(load_library().alice_codec_dev_requant_symbols(d_src_ptr or None, d_dst_ptr or None, n, 1 if wide else 0, step_from, step_to,
                                                          d_hist_ptr or None, stream or None))


# ---- banded format (.alc version 5) ----
# One frequency table per wavelet subband instead of one per channel: the pixels of the base version (2, 3 or 4) in fewer
# bytes at chunk sizes (the 12 636-byte header makes thumbnails larger).  Frame ranges, previews, rectangles, budgets and
# transcodes stay with the base versions: from_banded gives the base chunk back byte for byte.

BANDED_HEADER_BYTES = 12636


class _CBandedInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("frames", C.c_uint32), ("lane_symbols", C.c_uint32),
                ("wavelet", C.c_uint8), ("base", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("quant_step", C.c_int32 * 3), ("dead_zone", C.c_int32 * 3), ("num_symbols", C.c_uint32 * 3),
                ("n_blocks", C.c_uint32 * 24), ("payload_len", C.c_uint64 * 24)]


class BandedInfo:
    """The header fields of a version 5 container (alice_codec_banded_info: validated, no device needed).  n_blocks and
    payload_len have 24 entries: channel-major, band k = 4 bt + 2 by + bx ascending inside a channel."""

    def __init__(self, c: _CBandedInfo):
        self.width, self.height, self.frames = int(c.width), int(c.height), int(c.frames)
        self.lane_symbols = int(c.lane_symbols)
        self.wavelet_type = WaveletType(int(c.wavelet))
        self.base = int(c.base)
        self.quant_step = [int(v) for v in c.quant_step]
        self.dead_zone = [int(v) for v in c.dead_zone]
        self.num_symbols = [int(v) for v in c.num_symbols]
        self.n_blocks = [int(v) for v in c.n_blocks]
        self.payload_len = [int(v) for v in c.payload_len]

    def __repr__(self):
        return (f"BandedInfo({self.width}x{self.height}x{self.frames}, {self.wavelet_type.name}, base={self.base}, "
                f"lane_symbols={self.lane_symbols}, steps={self.quant_step}, payload={self.payload_len})")


def banded_info(data) -> BandedInfo:
    buf = _as_u8(data)
    c = _CBandedInfo()
    _check(load_library().alice_codec_banded_info(_p(buf, _u8p), buf.size, C.byref(c)))
    return BandedInfo(c)


def banded_stream_bound(n_band: int, lane_symbols: int = SPLIT_DEFAULT_LANE_SYMBOLS, base: int = 2) -> int:
    return int(load_library().alice_codec_banded_stream_bound(n_band, lane_symbols, _u8_arg(base, "base")))


def _banded_bytes(ptr, n) -> bytes:
    lib = load_library()
    if not ptr:
        _raise_last()
    try:
        return _copy_out(ptr, n.value).tobytes()
    finally:
        lib.alice_codec_data_free64(ptr, n.value)


def encode_banded(encoder: "FrameEncoder", rgb_frames, width: int, height: int, frames: int, lane_symbols: int = 0, base: int = 2) -> bytes:
    """One chunk as version 5 bytes of `base` (2: u8 symbols, 3: wide symbols, 4: wide symbols and the mirrored inverse), with
    the encoder's wavelet and quality.  It decodes to the pixels of the base version's chunk."""
    lib = load_library()
    buf = _as_u8(rgb_frames)
    _dims_u32(width, height, frames, lane_symbols)
    n = C.c_uint64(0)
    src = _p(buf, _u8p) if buf.size else C.cast(C.c_char_p(b""), _u8p)
    return _banded_bytes(lib.alice_codec_encode_banded(encoder._h, src, buf.size, width, height, frames, lane_symbols, _u8_arg(base, "base"),
                                                       C.byref(n)), n)


def decode_banded(data) -> np.ndarray:
    """The RGB bytes of a version 5 container."""
    lib = load_library()
    buf = _as_u8(data)
    n = C.c_uint64(0)
    ptr = lib.alice_codec_decode_banded(_p(buf, _u8p), buf.size, C.byref(n))
    if not ptr:
        _raise_last()
    return _adopt(ptr, n.value, lib.alice_codec_data_free64)


def to_banded(data, lane_symbols: int = 0) -> bytes:
    """A version 2, 3 or 4 container as the version 5 container of that base, from its symbols alone (no transform runs):
    byte for byte what encode_banded makes of the same input.  lane_symbols 0 keeps the source's."""
    buf = _as_u8(data)
    _dims_u32(lane_symbols)
    n = C.c_uint64(0)
    return _banded_bytes(load_library().alice_codec_to_banded(_p(buf, _u8p), buf.size, lane_symbols, C.byref(n)), n)


def from_banded(data, lane_symbols: int = 0) -> bytes:
    """A version 5 container as the container of its base version: from_banded(to_banded(x)) == x."""
    buf = _as_u8(data)
    _dims_u32(lane_symbols)
    n = C.c_uint64(0)
    return _banded_bytes(load_library().alice_codec_from_banded(_p(buf, _u8p), buf.size, lane_symbols, C.byref(n)), n)


def banded_encode_device(d_rgb_ptr: int, width: int, height: int, frames: int, n_chunks: int, wavelet_type: WaveletType,
                         quality: int, d_out_ptr: int, out_stride: int, qualities=None, lane_symbols: int = 0, base: int = 2,
                         stream: int = 0) -> np.ndarray:
    """n_chunks packed device chunks -> version 5 bytes of `base` at d_out_ptr + i * out_stride; returns the sizes."""
    sizes = np.zeros(n_chunks, np.uint64)
    q = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8).reshape(-1)
    if q is not None and q.size != n_chunks:
        raise ValueError("one quality per chunk")
    _dims_u32(width, height, frames, n_chunks, lane_symbols)
    _check(load_library().alice_codec_dev_encode_banded(d_rgb_ptr, width, height, frames, n_chunks, int(wavelet_type), quality,
                                                        None if q is None else _p(q, _u8p), lane_symbols, _u8_arg(base, "base"),
                                                        d_out_ptr, out_stride, _p(sizes, _u64p), stream or None))
    return sizes


def banded_decode_device(d_alc_ptr: int, alc_stride: int, sizes, d_rgb_out_ptr: int, stream: int = 0) -> None:
    s = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    _check(load_library().alice_codec_dev_decode_banded(d_alc_ptr, alc_stride, _p(s, _u64p), s.size, d_rgb_out_ptr, stream or None))


def _repack_device(fn: str, d_alc_ptr: int, alc_stride: int, sizes, d_out_ptr: int, out_stride: int, lane_symbols: int, stream: int):
    s = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    _dims_u32(lane_symbols)
    out = np.zeros(s.size, np.uint64)
    _check(getattr(load_library(), fn)(d_alc_ptr, alc_stride, _p(s, _u64p), s.size, lane_symbols, d_out_ptr, out_stride, _p(out, _u64p),
                                       stream or None))
    return out


def to_banded_device(d_alc_ptr: int, alc_stride: int, sizes, d_out_ptr: int, out_stride: int, lane_symbols: int = 0,
                     stream: int = 0) -> np.ndarray:
    """len(sizes) device containers of one version (2, 3 or 4), wavelet, shape and lane_symbols -> their version 5 twins at
    d_out_ptr + i * out_stride; returns the sizes."""
    return _repack_device("alice_codec_dev_to_banded", d_alc_ptr, alc_stride, sizes, d_out_ptr, out_stride, lane_symbols, stream)


def from_banded_device(d_alc_ptr: int, alc_stride: int, sizes, d_out_ptr: int, out_stride: int, lane_symbols: int = 0,
                       stream: int = 0) -> np.ndarray:
    """len(sizes) version 5 device containers of one base, wavelet, shape and lane_symbols -> their base chunks."""
    return _repack_device("alice_codec_dev_from_banded", d_alc_ptr, alc_stride, sizes, d_out_ptr, out_stride, lane_symbols, stream)


def band_histograms_device(d_symbols_ptr: int, width: int, height: int, frames: int, wide: bool, d_hist_ptr: int, stream: int = 0) -> None:
    """Stage call: the 3 x 8 x 256 u32 band histograms (wide: of min(z, 255)) of one chunk's 3 * padded device symbols."""
    _dims_u32(width, height, frames)
    _check(load_library().alice_codec_dev_band_histograms(d_symbols_ptr or None, width, height, frames, 1 if wide else 0,
                                                          d_hist_ptr or None, stream or None))


# ---- frame ranges and half-size previews of a version 5 chunk ----

def _banded_partial_host(fn: str, data, first: int, count: int) -> np.ndarray:
    lib = load_library()
    buf = _as_u8(data)
    _dims_u32(first, count)
    n = C.c_uint64(0)
    ptr = getattr(lib, fn)(_p(buf, _u8p), buf.size, first, count, C.byref(n))
    if not ptr:
        _raise_last()
    return _adopt(ptr, n.value, lib.alice_codec_data_free64)


def decode_banded_frames(data, first: int, count: int) -> np.ndarray:
    """The RGB bytes of frames [first, first + count) of a version 5 container, bit for bit decode_frames(from_banded(data),
    first, count): of every band only the blocks that hold coefficient planes of the range's window are read, uploaded (data
    may be an np.memmap) and entropy-decoded.  The end checks cover the blocks that are read."""
    return _banded_partial_host("alice_codec_decode_banded_frames", data, first, count)


def banded_frames_decode_device(d_alc_ptr: int, length: int, first: int, count: int, d_rgb_out_ptr: int, stream: int = 0) -> None:
    """decode_banded_frames of a device-resident container of `length` bytes into count packed frames at d_rgb_out_ptr."""
    _dims_u32(first, count)
    _check(load_library().alice_codec_dev_decode_banded_frames(d_alc_ptr, length, first, count, d_rgb_out_ptr, stream or None))


def decode_banded_preview(data, first: int, count: int) -> np.ndarray:
    """The half-resolution RGB bytes (count * qh * qw * 3, preview_dims) of frames [first, first + count) of a version 5
    container, bit for bit decode_preview(from_banded(data), first, count): bands 0 and 4 are the low-low quadrants, so only
    their blocks inside the window are read, uploaded and entropy-decoded, and no spatial inverse runs."""
    return _banded_partial_host("alice_codec_decode_banded_preview", data, first, count)


def banded_preview_decode_device(d_alc_ptr: int, length: int, first: int, count: int, d_rgb_out_ptr: int, stream: int = 0) -> None:
    """decode_banded_preview of a device-resident container of `length` bytes into count packed preview frames."""
    _dims_u32(first, count)
    _check(load_library().alice_codec_dev_decode_banded_preview(d_alc_ptr, length, first, count, d_rgb_out_ptr, stream or None))


def _test_last_banded_partial_stats(kind: str) -> tuple:
    """(a, b, blocks decoded over the channels and kept bands, payload bytes the host call uploaded, frames written, symbols
    stored over the three channels) of the calling thread's last banded frame-range (kind "frames") or preview decode."""
    out = np.zeros(6, np.uint64)
    getattr(load_library(), f"alice_codec_test_last_banded_{kind}_stats")(_p(out, _u64p))
    return tuple(int(v) for v in out)
