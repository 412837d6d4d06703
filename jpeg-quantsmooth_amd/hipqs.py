"""ctypes binding of libjpegqs_hip.so (include/jpegqs_hip.h)."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
MAXC = 4


class FLAGS:
    """JPEGQS_* algorithm flags, numerically the reference's (libjpegqs.h:14-32)."""
    DIAGONALS = 1
    JOINT_YUV = 2
    UPSAMPLE_UV = 4
    LOW_QUALITY = 8
    NO_REBALANCE = 16
    NO_REBALANCE_UV = 32
    TRANSCODE = 64
    MASK = 0x7F
    ITER_MAX = 100


def flags_for_quality(quality: int) -> int:
    """the jpegqs CLI's --quality -> flags mapping (reference quantsmooth.c:380-393)."""
    q = int(quality)
    flags = 0
    if q < 3:
        flags |= FLAGS.LOW_QUALITY
        q += 4
    if q >= 4:
        flags |= FLAGS.DIAGONALS
    if q >= 5:
        flags |= FLAGS.JOINT_YUV
    if q >= 6:
        flags |= FLAGS.UPSAMPLE_UV
    return flags


class QsHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libjpegqs_hip error {code}: {msg}")
        self.code = code


class Job(C.Structure):
    _fields_ = [
        ("ncomp", C.c_int32), ("colorspace", C.c_int32),
        ("image_width", C.c_int32), ("image_height", C.c_int32),
        ("wblk", C.c_int32 * MAXC), ("hblk", C.c_int32 * MAXC),
        ("hsamp", C.c_int32 * MAXC), ("vsamp", C.c_int32 * MAXC),
        ("has_quant", C.c_int32 * MAXC),
        ("quant", (C.c_uint16 * 64) * MAXC),
        ("coef", C.c_void_p * MAXC),
        ("coef_up", C.c_void_p * 2),
        ("up_wblk", C.c_int32), ("up_hblk", C.c_int32),
        ("out_hsamp0", C.c_int32), ("out_vsamp0", C.c_int32),
    ]


class PlaneRef(C.Structure):
    """qs_hip_plane_ref: one plane of a plane-set launch (device pointers)"""
    _fields_ = [("d_consts", C.c_void_p), ("d_coef", C.c_void_p), ("d_plane", C.c_void_p), ("d_status", C.c_void_p),
                ("wblk", C.c_int32), ("hblk", C.c_int32), ("luma", C.c_int32), ("band", C.c_int32)]


class PlaneRefs:
    """what HipQS.plane_refs() returns: the qs_hip_plane_ref array of a plane-set launch plus the PARALLEL array of second
    planes qs_hip_smooth_planes_next takes (None when no plane has one)"""
    def __init__(self, arr, nxt):
        self.arr, self.next = arr, nxt

    def __len__(self):
        return len(self.arr)

    def __getitem__(self, i):
        return self.arr[i]


class DeviceInfo(C.Structure):
    """qs_hip_device_info: what a device-resident job needs (qs_hip_device_job_info)"""
    _fields_ = [("workspace_bytes", C.c_size_t), ("up_wblk", C.c_int32), ("up_hblk", C.c_int32),
                ("out_hsamp0", C.c_int32), ("out_vsamp0", C.c_int32), ("static_stop", C.c_int32)]


class DecodeInfo(C.Structure):
    """qs_hip_decode_info: the output of one job of the device decode (qs_hip_decode_device_batch_info)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("layout", C.c_int32)]


class CompressInfo(C.Structure):
    """qs_hip_compress_info: the input of one job of the device compress and the blocks it writes
    (qs_hip_compress_device_batch_info)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("layout", C.c_int32),
                ("wblk", C.c_int32 * MAXC), ("hblk", C.c_int32 * MAXC)]


class CompressOpts(C.Structure):
    """qs_hip_compress_opts: the chroma downsampling of one job of the device compress (DOWNSAMPLE_BOX / DOWNSAMPLE_DCT)"""
    _fields_ = [("downsampling", C.c_int32), ("reserved", C.c_int32 * 3)]


class DecodeOpts(C.Structure):
    """qs_hip_decode_opts: the chroma upsampling of one job of the device decode (UPSAMPLE_DCT / UPSAMPLE_TRIANGLE)"""
    _fields_ = [("upsampling", C.c_int32)]


class DecodeScaleOpts(C.Structure):
    """qs_hip_decode_scale_opts: the chroma upsampling and the reduced size (scale_denom 1, 2, 4 or 8) of one job of the
    device decode"""
    _fields_ = [("upsampling", C.c_int32), ("scale_denom", C.c_int32)]


class HuffTable(C.Structure):
    """qs_hip_huff_table: bits[l] = codes of length l, huffval = the symbols by increasing code length"""
    _fields_ = [("bits", C.c_uint8 * 17), ("huffval", C.c_uint8 * 256)]


class HuffTables(C.Structure):
    """qs_hip_huff_tables: up to two DC and two AC tables of one job (has_* 0: the standard table)"""
    _fields_ = [("dc", HuffTable * 2), ("ac", HuffTable * 2), ("has_dc", C.c_uint8 * 2), ("has_ac", C.c_uint8 * 2)]


class EncodeInfo(C.Structure):
    """qs_hip_encode_info: one job of the device entropy coder (qs_hip_encode_device_batch_info)"""
    _fields_ = [("dc_tbl", C.c_int32 * MAXC), ("ac_tbl", C.c_int32 * MAXC), ("blocks_in_mcu", C.c_int32 * 2),
                ("max_segment_bytes", C.c_uint64)]


class EncodeFrame(C.Structure):
    """qs_hip_encode_frame: the device bytes around the tables and the scan of one job, per geometry variant"""
    _fields_ = [("d_head", C.c_void_p * 2), ("head_bytes", C.c_uint32 * 2), ("d_mid", C.c_void_p * 2),
                ("mid_bytes", C.c_uint32 * 2)]


class EncodeOpts(C.Structure):
    """qs_hip_encode_opts: the restart interval of one job (in MCUs, or in MCU rows when restart_in_rows > 0)"""
    _fields_ = [("restart_interval", C.c_int32), ("restart_in_rows", C.c_int32)]


MAX_SCANS = 256                  # QS_HIP_MAX_SCANS: scans of one progressive script
PROG_REFINE = 1                  # QS_HIP_PROG_REFINE: qs_hip_encode_prog_opts.flags, refinement scans are written


class EncodeScan(C.Structure):
    """qs_hip_encode_scan: one scan of a progressive script (jpeg_scan_info)"""
    _fields_ = [("ncomp", C.c_int32), ("comp", C.c_int32 * 4), ("Ss", C.c_int32), ("Se", C.c_int32), ("Ah", C.c_int32),
                ("Al", C.c_int32)]


class EncodeProgOpts(C.Structure):
    """qs_hip_encode_prog_opts: the script and the restart settings of one job of the progressive run"""
    _fields_ = [("scans", C.POINTER(EncodeScan)), ("nscans", C.c_int32), ("restart_interval", C.c_int32),
                ("restart_in_rows", C.c_int32), ("component_id", C.c_int32 * MAXC), ("flags", C.c_int32)]


class EncodeProgInfo(C.Structure):
    """qs_hip_encode_prog_info: one job of the progressive run (qs_hip_encode_progressive_device_batch_info)"""
    _fields_ = [("nscans", C.c_int32), ("mcus", C.c_int32 * MAX_SCANS), ("interval", C.c_int32 * MAX_SCANS),
                ("max_body_bytes", C.c_uint64)]


class ReadOpts(C.Structure):
    """qs_hip_read_opts: the Huffman tables of a file by DHT id (has_* 0: the standard table, ids 0 / 1), Td / Ta of each
    component and the DRI value"""
    _fields_ = [("dc", HuffTable * 4), ("ac", HuffTable * 4), ("has_dc", C.c_uint8 * 4), ("has_ac", C.c_uint8 * 4),
                ("dc_tbl", C.c_int32 * MAXC), ("ac_tbl", C.c_int32 * MAXC), ("restart_interval", C.c_int32)]


class ReadInfo(C.Structure):
    """qs_hip_read_info: one job of the device scan reader (qs_hip_read_device_batch_info)"""
    _fields_ = [("blocks_in_mcu", C.c_int32), ("mcus", C.c_int32), ("intervals", C.c_int32),
                ("blocks_per_interval", C.c_int64)]


class ReadSplitInfo(C.Structure):
    """qs_hip_read_split_info: one job of the scan reader's split route (qs_hip_read_split_device_batch_info)"""
    _fields_ = ReadInfo._fields_ + [("max_segments", C.c_int64)]


class ReadProgScan(C.Structure):
    """qs_hip_read_prog_scan: one scan of a progressive file -- its jpeg_scan_info record, Td / Ta of its components, the
    DHT tables and the DRI value in effect at its SOS, the offset of the first byte behind its SOS header"""
    _fields_ = [("scan", EncodeScan), ("dc_tbl", C.c_int32 * MAXC), ("ac_tbl", C.c_int32 * MAXC), ("dc", HuffTable * 4),
                ("ac", HuffTable * 4), ("has_dc", C.c_uint8 * 4), ("has_ac", C.c_uint8 * 4), ("restart_interval", C.c_int32),
                ("offset", C.c_uint64)]


class ReadProgOpts(C.Structure):
    """qs_hip_read_prog_opts: the scans of one progressive file (jpeg_file.parse_progressive)"""
    _fields_ = [("scans", C.POINTER(ReadProgScan)), ("nscans", C.c_int32)]


class ReadProgInfo(C.Structure):
    """qs_hip_read_prog_info: one job of the scan reader's progressive route (qs_hip_read_prog_device_batch_info)"""
    _fields_ = [("nscans", C.c_int32), ("levels", C.c_int32), ("mcus", C.c_int32 * MAX_SCANS),
                ("intervals", C.c_int32 * MAX_SCANS)]


READ_SPLIT_BYTES = 256           # QS_HIP_READ_SPLIT_BYTES: stuffed bytes of a restart interval one lane decodes
READ_SPLIT_ROUNDS = 17           # QS_HIP_READ_SPLIT_ROUNDS: synchronisation launches of the split route

MAX_PLANES = 56
COMPRESS_CHUNK = 44              # QS_HIP_COMPRESS_CHUNK: jobs per launch of the device compress
DOWNSAMPLE_BOX = 0               # QS_HIP_DOWNSAMPLE_BOX: do_fancy_downsampling = FALSE
DOWNSAMPLE_DCT = 1               # QS_HIP_DOWNSAMPLE_DCT: libjpeg 9's default, 2x chroma through 16-point scaled DCTs
DOWNSAMPLING = {"box": DOWNSAMPLE_BOX, "dct": DOWNSAMPLE_DCT}
DECODE_CHUNK = 44                # QS_HIP_DECODE_CHUNK: jobs per launch of the device decode
UPSAMPLE_DCT = 0                 # QS_HIP_UPSAMPLE_DCT: libjpeg 7..9, DCT-scaled chroma (the decode without opts)
UPSAMPLE_TRIANGLE = 1            # QS_HIP_UPSAMPLE_TRIANGLE: libjpeg-turbo / 6b, 8x8 islow + jdsample.c's triangle filters
UPSAMPLING = {"dct": UPSAMPLE_DCT, "triangle": UPSAMPLE_TRIANGLE}
PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int)

# every symbol include/jpegqs_hip.h declares: (restype, argtypes)
ABI = {
    "qs_hip_do_quantsmooth": (C.c_int, [C.POINTER(Job), C.c_int, C.c_int, C.c_int, PROGRESS_FN, C.c_void_p]),
    "qs_hip_do_quantsmooth_batch": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "qs_hip_do_quantsmooth_rows": (C.c_int, [C.POINTER(Job), C.POINTER(C.POINTER(C.c_void_p)), C.c_int, C.c_int, C.c_int,
                                          PROGRESS_FN, C.c_void_p]),
    "qs_hip_set_devices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "qs_hip_set_shard_schedule": (C.c_int, [C.c_int]),
    "qs_hip_do_quantsmooth_band": (C.c_int, [C.POINTER(Job), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_do_quantsmooth_sharded": (C.c_int, [C.POINTER(Job), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "qs_hip_band_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "qs_hip_colour_band_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4),
    "qs_hip_band_halo_rows": (C.c_int, [C.c_int, C.c_int] + [C.POINTER(C.c_size_t)] * 5),
    "qs_hip_prewarm": (C.c_int, [C.POINTER(Job), C.c_int, C.c_int]),
    "qs_hip_progress_calls": (C.c_int, [C.POINTER(Job), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]),
    "qs_hip_device_job_info": (C.c_int, [C.POINTER(Job), C.c_int, C.c_int, C.POINTER(DeviceInfo)]),
    "qs_hip_device_job_prepare": (C.c_int, [C.POINTER(Job), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_do_quantsmooth_device": (C.c_int, [C.POINTER(Job), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_void_p]),
    "qs_hip_device_batch_info": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_int, C.c_int, C.POINTER(DeviceInfo),
                                            C.POINTER(C.c_size_t)]),
    "qs_hip_device_batch_prepare": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                               C.c_void_p]),
    "qs_hip_do_quantsmooth_device_batch": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                      C.c_size_t, C.c_void_p, C.c_void_p]),
    "qs_hip_decode_device_batch_info": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(DecodeInfo),
                                                   C.POINTER(C.c_size_t)]),
    "qs_hip_decode_device_batch_prepare": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_void_p, C.c_size_t,
                                                      C.c_void_p]),
    "qs_hip_decode_device_batch": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_void_p, C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_decode_device_batch_info_opts": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                        C.POINTER(C.POINTER(DecodeOpts)), C.POINTER(DecodeInfo),
                                                        C.POINTER(C.c_size_t)]),
    "qs_hip_decode_device_batch_prepare_opts": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                           C.POINTER(C.POINTER(DecodeOpts)), C.c_void_p, C.c_size_t,
                                                           C.c_void_p]),
    "qs_hip_decode_device_batch_info_scaled": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                          C.POINTER(C.POINTER(DecodeScaleOpts)), C.POINTER(DecodeInfo),
                                                          C.POINTER(C.c_size_t)]),
    "qs_hip_decode_device_batch_prepare_scaled": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                             C.POINTER(C.POINTER(DecodeScaleOpts)), C.c_void_p, C.c_size_t,
                                                             C.c_void_p]),
    "qs_hip_encode_device_batch_info": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(EncodeInfo),
                                                   C.POINTER(C.c_size_t)]),
    "qs_hip_encode_device_batch_prepare": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(C.POINTER(HuffTables)),
                                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_encode_device_batch": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_void_p, C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_void_p]),
    "qs_hip_encode_device_batch_histogram": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_encode_device_batch_info_opts": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                        C.POINTER(C.POINTER(EncodeOpts)), C.POINTER(EncodeInfo),
                                                        C.POINTER(C.c_size_t)]),
    "qs_hip_encode_device_batch_prepare_opts": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                           C.POINTER(C.POINTER(HuffTables)),
                                                           C.POINTER(C.POINTER(EncodeOpts)), C.c_void_p, C.c_size_t,
                                                           C.c_void_p]),
    "qs_hip_huff_optimal_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "qs_hip_encode_files_scratch_bytes": (C.c_size_t, [C.c_int]),
    "qs_hip_encode_device_batch_files": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(EncodeFrame), C.c_int,
                                                    C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                    C.c_void_p]),
    "qs_hip_encode_progressive_device_batch_info": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                               C.POINTER(C.POINTER(EncodeProgOpts)),
                                                               C.POINTER(EncodeProgInfo), C.POINTER(C.c_size_t),
                                                               C.POINTER(C.c_size_t)]),
    "qs_hip_encode_progressive_device_batch_prepare": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                                  C.POINTER(C.POINTER(EncodeProgOpts)), C.c_void_p,
                                                                  C.c_size_t, C.c_void_p]),
    "qs_hip_encode_progressive_device_batch_files": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(EncodeFrame),
                                                                C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                C.c_size_t, C.c_void_p]),
    "qs_hip_read_device_batch_info": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(C.POINTER(ReadOpts)),
                                                 C.POINTER(ReadInfo), C.POINTER(C.c_size_t)]),
    "qs_hip_read_device_batch_prepare": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(C.POINTER(ReadOpts)),
                                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_read_device_batch": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_read_split_device_batch_info": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(C.POINTER(ReadOpts)),
                                                       C.POINTER(ReadSplitInfo), C.POINTER(C.c_size_t)]),
    "qs_hip_read_split_device_batch_prepare": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(C.POINTER(ReadOpts)),
                                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_read_split_device_batch": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_read_prog_device_batch_info": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                      C.POINTER(C.POINTER(ReadProgOpts)), C.POINTER(ReadProgInfo),
                                                      C.POINTER(C.c_size_t)]),
    "qs_hip_read_prog_device_batch_prepare": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                         C.POINTER(C.POINTER(ReadProgOpts)), C.c_void_p, C.c_size_t,
                                                         C.c_void_p]),
    "qs_hip_read_prog_device_batch": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(C.c_void_p),
                                                 C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_compress_device_batch_info": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_int, C.POINTER(CompressInfo),
                                                     C.POINTER(C.c_size_t)]),
    "qs_hip_compress_device_batch_prepare": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                        C.c_void_p]),
    "qs_hip_compress_device_batch_info_opts": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                          C.POINTER(C.POINTER(CompressOpts)), C.POINTER(CompressInfo),
                                                          C.POINTER(C.c_size_t)]),
    "qs_hip_compress_device_batch_prepare_opts": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int,
                                                             C.POINTER(C.POINTER(CompressOpts)), C.c_void_p, C.c_size_t,
                                                             C.c_void_p]),
    "qs_hip_compress_device_batch": (C.c_int, [C.POINTER(C.POINTER(Job)), C.c_int, C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t, C.c_void_p]),
    "qs_hip_huff_optimal": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "qs_hip_huff_standard": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "qs_hip_free": (None, [C.c_void_p]),
    "qs_hip_release_cache": (None, []),
    "qs_hip_device_count": (C.c_int, []),
    "qs_hip_last_error": (C.c_char_p, []),
    "qs_hip_consts_bytes": (C.c_size_t, []),
    "qs_hip_plane_pitch": (C.c_size_t, [C.c_int]),
    "qs_hip_plane_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "qs_hip_plane_row_offset": (C.c_size_t, [C.c_int, C.c_int]),
    "qs_hip_consts_build": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint16), C.c_int]),
    "qs_hip_idct_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "qs_hip_smooth_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_smooth_plane_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_smooth_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_idct_planes": (C.c_int, [C.POINTER(PlaneRef), C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_smooth_planes": (C.c_int, [C.POINTER(PlaneRef), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_smooth_planes_next": (C.c_int, [C.POINTER(PlaneRef), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_abi_version": (C.c_int, []),
    "qs_hip_joint_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_lowq_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_downsample_plane": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_upsample_pitch": (C.c_size_t, [C.c_int, C.c_int]),
    "qs_hip_upsample_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "qs_hip_upsample_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_upsample_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                       C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_fdct_plane": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_clamp_plane": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "qs_hip_dequant_plane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
}


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so (SONAME libamdhip64.so.7, but requested by torch under the
    unversioned name), so loading our library first would pull in /opt/rocm's
    copy and torch would later load a SECOND runtime that sees no GPUs.  If a
    torch install is present, map its copy first; our NEEDED libamdhip64.so.7
    then resolves to it by SONAME and torch finds the same file by inode."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = Path(spec.origin).parent / "lib" / "libamdhip64.so"
    if cand.exists():
        try:
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib_path() -> Path:
    """the in-tree library; QS_HIP_LIB points measurement runs at an A/B build (tools/build_variants.sh)"""
    import os
    return Path(os.environ["QS_HIP_LIB"]) if os.environ.get("QS_HIP_LIB") else PKG_DIR / "libjpegqs_hip.so"


def load_library(path: Path | None = None) -> C.CDLL:
    """dlopen the HIP library; raises (no fallback) when it has not been built."""
    p = Path(path) if path else lib_path()
    if not p.exists():
        raise FileNotFoundError(
            f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C {PKG_DIR / 'csrc'}`; there is no CPU fallback")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(str(p))
    for name, (res, args) in ABI.items():
        f = getattr(lib, name)  # AttributeError if the ABI is incomplete
        f.restype = res
        f.argtypes = args
    return lib


def _ptr_array(rec, records, n, message):
    """the array of pointers to `rec` records a batch call of n jobs takes, one slot at least; an entry None stays NULL.
    records None: None, the call without them, where the ABI allows it.  Anything but n records: ValueError(message)"""
    if records is None:
        return None
    if len(records) != n:
        raise ValueError(message)
    return (C.POINTER(rec) * max(1, n))(*[None if r is None else C.pointer(r) for r in records])


def _named_ptrs(rec, field, names, what, opts, n):
    """opts: one entry per job -- None (the call's default mode), a name of `names`, one of its values or a `rec` -> (the
    pointer array, what it points to: keep it alive over the call); `what` and `field` word the refusals"""
    if len(opts) != n:
        raise ValueError(f"{what} opts: {len(opts)} entries for {n} jobs")
    keep = []
    for o in opts:
        if o is not None and not isinstance(o, rec):
            if isinstance(o, str):
                if o not in names:
                    raise ValueError(f"{what} opts: {field} {o!r} (one of {sorted(names)})")
                o = names[o]
            o = rec(**{field: int(o)})
        keep.append(o)
    return _ptr_array(rec, keep, n, None), keep


_DECODE_MODES = (DecodeOpts, "upsampling", UPSAMPLING, "decode")             # what _named_ptrs takes for decode opts
_COMPRESS_MODES = (CompressOpts, "downsampling", DOWNSAMPLING, "compress")   # ... and for compress opts


def _fill_huff(tabs, arr, has, ids, who):
    """tabs = {id: (bits[17], huffval)} or None into the HuffTable array `arr`, has[id] = 1 for each; ids: the ids the
    record has room for"""
    for k, (bits, vals) in (tabs or {}).items():
        if k not in ids or len(bits) != 17 or len(vals) > 256:
            raise ValueError(f"{who}: table {ids[0]}{' or ' if len(ids) == 2 else '..'}{ids[-1]}, bits[17], at most 256 "
                             f"symbols")
        arr[k].bits[:] = [int(b) for b in bits]
        for i, v in enumerate(vals):
            arr[k].huffval[i] = int(v)
        has[k] = 1


def _c_array(ctype, values):
    """values (addresses, sizes, pitches) as the C array a batch call takes, one slot at least"""
    return (ctype * max(1, len(values)))(*values)


def _info_dict(rec):
    """an info record of plain integers as a dict"""
    return {f: int(getattr(rec, f)) for f, _ in rec._fields_}


class HipQS:
    """Thin object wrapper: job layer on numpy arrays, plane layer on device pointers."""

    def __init__(self, path: Path | None = None):
        self.lib = load_library(path)

    # -- helpers ---------------------------------------------------------------
    def _check(self, rc: int) -> int:
        if rc < 0:
            raise QsHipError(rc, self.lib.qs_hip_last_error().decode(errors="replace"))
        return rc

    def device_count(self) -> int:
        return self.lib.qs_hip_device_count()

    def consts_bytes(self) -> int:
        return self.lib.qs_hip_consts_bytes()

    def plane_pitch(self, wblk: int) -> int:
        return self.lib.qs_hip_plane_pitch(wblk)

    def plane_bytes(self, wblk: int, hblk: int) -> int:
        return self.lib.qs_hip_plane_bytes(wblk, hblk)

    def plane_row_offset(self, wblk: int, y: int) -> int:
        return self.lib.qs_hip_plane_row_offset(wblk, y)

    def consts_build(self, quant, flags: int) -> np.ndarray:
        """host-side constant block (uint8 array) for one component"""
        q = np.ascontiguousarray(quant, dtype=np.uint16)
        out = np.zeros(self.consts_bytes(), dtype=np.uint8)
        self._check(self.lib.qs_hip_consts_build(out.ctypes.data, (C.c_uint16 * q.size).from_buffer_copy(q), flags))
        return out

    # -- band arithmetic (one definition, shared with csrc/qs_shard.cpp) ----------
    def band_rows(self, hblk: int, nbands: int, band: int, align: int = 1):
        r0, r1 = C.c_int(0), C.c_int(0)
        self._check(self.lib.qs_hip_band_rows(hblk, nbands, band, align, C.byref(r0), C.byref(r1)))
        return r0.value, r1.value

    def colour_band_rows(self, hblk_luma: int, hblk_chroma: int, v_samp: int, nbands: int, band: int):
        v = [C.c_int(0) for _ in range(4)]
        self._check(self.lib.qs_hip_colour_band_rows(hblk_luma, hblk_chroma, v_samp, nbands, band, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def band_halo_rows(self, wblk: int, hblk: int):
        """-> (send_top, send_bot, recv_top, recv_bot, nbytes): byte offsets inside a band's pixel plane"""
        v = [C.c_size_t(0) for _ in range(5)]
        self._check(self.lib.qs_hip_band_halo_rows(wblk, hblk, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # -- job layer -------------------------------------------------------------
    @staticmethod
    def _make_job(coefs, quants, hsamp=None, vsamp=None, colorspace=None, image_size=None):
        n = len(coefs)
        job = Job()
        job.ncomp = n
        job.colorspace = colorspace if colorspace is not None else (3 if n == 3 else 1)
        hsamp = hsamp or [1] * n
        vsamp = vsamp or [1] * n
        work = []
        for ci in range(n):
            a = np.ascontiguousarray(coefs[ci], dtype=np.int16).copy()
            assert a.ndim == 3 and a.shape[2] == 64
            work.append(a)
            job.hblk[ci], job.wblk[ci] = a.shape[0], a.shape[1]
            job.hsamp[ci], job.vsamp[ci] = hsamp[ci], vsamp[ci]
            job.coef[ci] = a.ctypes.data
            if quants[ci] is not None:
                job.has_quant[ci] = 1
                for i in range(64):
                    job.quant[ci][i] = int(quants[ci][i])
        if image_size is None:
            mh, mv = max(hsamp), max(vsamp)
            image_size = (work[0].shape[1] * 8 * mh // hsamp[0], work[0].shape[0] * 8 * mv // vsamp[0])
        job.image_width, job.image_height = image_size
        return job, work

    def _job_result(self, job, work, quants, ret):
        up = job.up_wblk > 0
        if up:
            for j in range(2):
                cnt = job.up_wblk * job.up_hblk * 64
                buf = (C.c_int16 * cnt).from_address(job.coef_up[j])
                work[1 + j] = np.frombuffer(buf, dtype=np.int16).reshape(job.up_hblk, job.up_wblk, 64).copy()
                self.lib.qs_hip_free(job.coef_up[j])
        qout = [np.array(job.quant[ci][:], dtype=np.uint16) if quants[ci] is not None else None
                for ci in range(job.ncomp)]
        return dict(ret=ret, coefs=work, quants=qout, up=up,
                    hsamp0=job.out_hsamp0, vsamp0=job.out_vsamp0)

    def do_quantsmooth(self, coefs, quants, flags, niter, *, hsamp=None, vsamp=None,
                       colorspace=None, image_size=None, progprec=0, progress=None, threads=None, devices=None):
        """Whole do_quantsmooth() on copies of the inputs; same calling convention
        and result dict as the test oracles (`threads` is accepted and ignored:
        the GPU has no use for jpegqs_control_t.threads).  devices=[...]: cut the job
        over these HIP devices (qs_hip_do_quantsmooth_sharded; an ordinal may repeat)."""
        job, work = self._make_job(coefs, quants, hsamp, vsamp, colorspace, image_size)
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            ret = self._check(self.lib.qs_hip_do_quantsmooth_sharded(C.byref(job), flags, niter, arr, len(devices)))
            return self._job_result(job, work, quants, ret)
        cb = PROGRESS_FN(progress) if progress else C.cast(None, PROGRESS_FN)
        ret = self._check(self.lib.qs_hip_do_quantsmooth(C.byref(job), flags, niter, progprec, cb, None))
        return self._job_result(job, work, quants, ret)

    def progress_calls(self, coefs, quants, niter, progprec=0, **kw):
        """qs_hip_progress_calls: [(cur, max), ...] the progress callback of this job will see (no device needed)"""
        job, _work = self._make_job(coefs, quants, kw.get("hsamp"), kw.get("vsamp"), kw.get("colorspace"), kw.get("image_size"))
        out = (C.c_int * 4096)()
        mx = C.c_int(0)
        n = self._check(self.lib.qs_hip_progress_calls(C.byref(job), niter, progprec, out, 4096, C.byref(mx)))
        return [(int(out[k]), int(mx.value)) for k in range(min(n, 4096))]

    def set_devices(self, devices):
        """qs_hip_set_devices: the device list large jobs are spread over ([] = default)"""
        arr = (C.c_int * max(1, len(devices)))(*devices)
        self._check(self.lib.qs_hip_set_devices(arr, len(devices)))

    def do_quantsmooth_band(self, coefs, quants, flags, niter, rank, nranks, comm=None, **kw):
        """qs_hip_do_quantsmooth_band: this rank's band of a job whose halo rows travel through RCCL (`comm`: ncclComm_t as int)"""
        job, work = self._make_job(coefs, quants, kw.get("hsamp"), kw.get("vsamp"), kw.get("colorspace"), kw.get("image_size"))
        ret = self._check(self.lib.qs_hip_do_quantsmooth_band(C.byref(job), flags, niter, rank, nranks, comm))
        return self._job_result(job, work, quants, ret)

    def set_shard_schedule(self, schedule: int):
        """qs_hip_set_shard_schedule: 0 = one halo row per iteration, 1 = deep halo (no exchange), -1 = default"""
        self._check(self.lib.qs_hip_set_shard_schedule(schedule))

    def do_quantsmooth_batch(self, jobs, flags, niter):
        """qs_hip_do_quantsmooth_batch: `jobs` = list of dicts with the keyword
        arguments of do_quantsmooth (coefs, quants and optionally hsamp, vsamp,
        colorspace, image_size) -> list of result dicts in the same order
        (ret < 0: that job failed with this error code)"""
        made = [self._make_job(j["coefs"], j["quants"], j.get("hsamp"), j.get("vsamp"),
                               j.get("colorspace"), j.get("image_size")) for j in jobs]
        ptrs = self._job_ptrs([m[0] for m in made])
        results = (C.c_int * max(1, len(made)))()
        self._check(self.lib.qs_hip_do_quantsmooth_batch(ptrs, len(made), flags, niter, results))
        return [self._job_result(m[0], m[1], j["quants"], int(results[i])) for i, (m, j) in enumerate(zip(made, jobs))]

    # -- device-resident job (device pointers as ints, stream as int or None) ---
    @staticmethod
    def device_job(coef_ptrs, shapes, quants, *, hsamp=None, vsamp=None, colorspace=None, image_size=None,
                   coef_up=None) -> Job:
        """a qs_hip_job over DEVICE arrays: coef_ptrs[ci] = device address of component ci's (hblk, wblk, 64) int16
        blocks, shapes[ci] = (hblk, wblk); quants[ci] = 64 quantisers (natural order) or None; coef_up = the two device
        arrays for UPSAMPLE_UV's replacement chroma (device_job_info tells whether and how large)"""
        n = len(coef_ptrs)
        if not 1 <= n <= MAXC or len(shapes) != n or len(quants) != n:
            raise ValueError("device_job: 1..4 components, one shape and one quant table (or None) each")
        job = Job()
        job.ncomp = n
        job.colorspace = colorspace if colorspace is not None else (3 if n == 3 else 1)
        hsamp = hsamp or [1] * n
        vsamp = vsamp or [1] * n
        for ci in range(n):
            job.hblk[ci], job.wblk[ci] = int(shapes[ci][0]), int(shapes[ci][1])
            job.hsamp[ci], job.vsamp[ci] = int(hsamp[ci]), int(vsamp[ci])
            job.coef[ci] = int(coef_ptrs[ci]) if coef_ptrs[ci] else None
            if quants[ci] is not None:
                job.has_quant[ci] = 1
                for i in range(64):
                    job.quant[ci][i] = int(quants[ci][i])
        if image_size is None:
            mh, mv = max(hsamp), max(vsamp)
            image_size = (job.wblk[0] * 8 * mh // hsamp[0], job.hblk[0] * 8 * mv // vsamp[0])
        job.image_width, job.image_height = int(image_size[0]), int(image_size[1])
        if coef_up is not None:
            job.coef_up[0], job.coef_up[1] = coef_up[0], coef_up[1]
        return job

    def device_job_info(self, job: Job, flags: int, niter: int) -> dict:
        """qs_hip_device_job_info (no device needed) -> dict(workspace_bytes, up_wblk, up_hblk, out_hsamp0, out_vsamp0,
        static_stop)"""
        info = DeviceInfo()
        self._check(self.lib.qs_hip_device_job_info(C.byref(job), flags, niter, C.byref(info)))
        return _info_dict(info)

    def device_job_prepare(self, job: Job, flags: int, niter: int, d_workspace: int, nbytes: int, stream=None) -> None:
        """qs_hip_device_job_prepare: the constant blocks into the workspace (synchronises `stream`; not inside a capture)"""
        self._check(self.lib.qs_hip_device_job_prepare(C.byref(job), flags, niter, d_workspace, nbytes, stream))

    def do_quantsmooth_device(self, job: Job, flags: int, niter: int, d_workspace: int, nbytes: int, d_stop: int,
                              stream=None) -> None:
        """qs_hip_do_quantsmooth_device: enqueue the whole job on `stream`; the reference's return value lands in the
        device int32 at d_stop.  Sets job.quant to 1 and job.up_* / out_*samp0 like the job layer."""
        self._check(self.lib.qs_hip_do_quantsmooth_device(C.byref(job), flags, niter, d_workspace, nbytes, d_stop, stream))

    # -- device-resident batch (a list of device_job() Jobs) -------------------------
    @staticmethod
    def _job_ptrs(jobs):
        return _ptr_array(Job, jobs, len(jobs), None)

    def device_batch_info(self, jobs, flags: int, niter: int):
        """qs_hip_device_batch_info (no device needed) -> (list of per-job dicts as device_job_info returns them,
        the batch's workspace bytes)"""
        per = (DeviceInfo * max(1, len(jobs)))()
        total = C.c_size_t(0)
        self._check(self.lib.qs_hip_device_batch_info(self._job_ptrs(jobs), len(jobs), flags, niter, per, C.byref(total)))
        return [_info_dict(p) for p in per[:len(jobs)]], int(total.value)

    def device_batch_prepare(self, jobs, flags: int, niter: int, d_workspace: int, nbytes: int, stream=None) -> None:
        """qs_hip_device_batch_prepare: constants and descriptor tables into the workspace (synchronises `stream`; not
        inside a capture)"""
        self._check(self.lib.qs_hip_device_batch_prepare(self._job_ptrs(jobs), len(jobs), flags, niter, d_workspace,
                                                         nbytes, stream))

    def do_quantsmooth_device_batch(self, jobs, flags: int, niter: int, d_workspace: int, nbytes: int, d_stop: int,
                                    stream=None) -> None:
        """qs_hip_do_quantsmooth_device_batch: enqueue every job on `stream`; job i's return value lands in the device
        int32 at d_stop + 4 * i.  Sets each job's quant to 1 and up_* / out_*samp0 like the single-job call."""
        self._check(self.lib.qs_hip_do_quantsmooth_device_batch(self._job_ptrs(jobs), len(jobs), flags, niter,
                                                                d_workspace, nbytes, d_stop, stream))

    # -- device decode to pixels (a list of device_job() Jobs) ---------------------------
    @classmethod
    def _decode_scale_ptrs(cls, opts, scales, n):
        """scales: one scale_denom per job (None: full size); opts as decode_batch_info takes them or None -> (the pointer
        array of DecodeScaleOpts, what it points to)"""
        if len(scales) != n:
            raise ValueError(f"decode scales: {len(scales)} entries for {n} jobs")
        _arr, modes = _named_ptrs(*_DECODE_MODES, [None] * n if opts is None else opts, n)
        keep = []
        for mode, d in zip(modes, scales):
            if isinstance(d, DecodeScaleOpts):
                keep.append(d)
                continue
            rec = DecodeScaleOpts()
            rec.upsampling = UPSAMPLE_DCT if mode is None else mode.upsampling
            rec.scale_denom = 1 if d is None else int(d)
            keep.append(rec)
        return _ptr_array(DecodeScaleOpts, keep, n, None), keep

    def decode_batch_info(self, jobs, opts=None, scales=None):
        """qs_hip_decode_device_batch_info[_opts / _scaled] (no device needed) -> (list of dict(width, height, channels,
        layout), the batch's workspace bytes).  opts: None (the call without opts: every job in the dct mode), or one
        entry per job: None, "dct", "triangle" (libjpeg-turbo's triangle-filter chroma upsampling) or a DecodeOpts.
        scales: None, or one scale_denom per job (1, 2, 4, 8; None = 1): libjpeg 9's reduced sizes, through the _scaled
        call; width and height are then the scaled output's"""
        per = (DecodeInfo * max(1, len(jobs)))()
        total = C.c_size_t(0)
        if scales is not None:
            arr, _keep = self._decode_scale_ptrs(opts, scales, len(jobs))
            self._check(self.lib.qs_hip_decode_device_batch_info_scaled(self._job_ptrs(jobs), len(jobs), arr, per,
                                                                        C.byref(total)))
        elif opts is None:
            self._check(self.lib.qs_hip_decode_device_batch_info(self._job_ptrs(jobs), len(jobs), per, C.byref(total)))
        else:
            arr, _keep = _named_ptrs(*_DECODE_MODES, opts, len(jobs))
            self._check(self.lib.qs_hip_decode_device_batch_info_opts(self._job_ptrs(jobs), len(jobs), arr, per,
                                                                      C.byref(total)))
        return [_info_dict(p) for p in per[:len(jobs)]], int(total.value)

    def decode_batch_prepare(self, jobs, d_workspace: int, nbytes: int, stream=None, opts=None, scales=None) -> None:
        """qs_hip_decode_device_batch_prepare[_opts / _scaled]: geometry, modes, scales and tables into the workspace
        (synchronises `stream`; not inside a capture); opts and scales as decode_batch_info takes them"""
        if scales is not None:
            arr, _keep = self._decode_scale_ptrs(opts, scales, len(jobs))
            self._check(self.lib.qs_hip_decode_device_batch_prepare_scaled(self._job_ptrs(jobs), len(jobs), arr,
                                                                           d_workspace, nbytes, stream))
        elif opts is None:
            self._check(self.lib.qs_hip_decode_device_batch_prepare(self._job_ptrs(jobs), len(jobs), d_workspace, nbytes,
                                                                    stream))
        else:
            arr, _keep = _named_ptrs(*_DECODE_MODES, opts, len(jobs))
            self._check(self.lib.qs_hip_decode_device_batch_prepare_opts(self._job_ptrs(jobs), len(jobs), arr,
                                                                         d_workspace, nbytes, stream))

    def decode_batch(self, jobs, d_stop, d_out, pitch, d_workspace: int, nbytes: int, stream=None) -> None:
        """qs_hip_decode_device_batch: enqueue the decode of every job (one launch per 44 jobs); d_out[i] = device
        address of job i's output, pitch[i] = bytes between its rows; d_stop: the device int32[njobs] a
        smoothing run wrote (picks each UPSAMPLE_UV job's geometry on the device) or None"""
        self._check(self.lib.qs_hip_decode_device_batch(self._job_ptrs(jobs), len(jobs), d_stop, _c_array(C.c_void_p, d_out),
                                                        _c_array(C.c_size_t, pitch), d_workspace, nbytes, stream))

    # -- device compress of pixels (a list of device_job() Jobs over the arrays to fill) ---
    def compress_batch_info(self, jobs, fancy: bool = False, opts=None):
        """qs_hip_compress_device_batch_info[_opts] (no device needed) -> (list of dict(width, height, channels, layout,
        wblk, hblk: libjpeg's block geometry per component), the batch's workspace bytes).  opts: None (the call without
        opts: every job in the box mode), or one entry per job: None, "box", "dct" (libjpeg 9's default DCT-scaled
        chroma downsampling) or a CompressOpts.  fancy: the old argument, still refused (QS_HIP_ENOTSUP)"""
        per = (CompressInfo * max(1, len(jobs)))()
        total = C.c_size_t(0)
        if opts is None or fancy:
            self._check(self.lib.qs_hip_compress_device_batch_info(self._job_ptrs(jobs), len(jobs), int(bool(fancy)), per,
                                                                   C.byref(total)))
        else:
            arr, _keep = _named_ptrs(*_COMPRESS_MODES, opts, len(jobs))
            self._check(self.lib.qs_hip_compress_device_batch_info_opts(self._job_ptrs(jobs), len(jobs), arr, per,
                                                                        C.byref(total)))
        out = []
        for i, job in enumerate(jobs):
            n = int(job.ncomp)
            out.append(dict(width=int(per[i].width), height=int(per[i].height), channels=int(per[i].channels),
                            layout=int(per[i].layout), wblk=list(per[i].wblk[:n]), hblk=list(per[i].hblk[:n])))
        return out, int(total.value)

    def compress_batch_prepare(self, jobs, d_workspace: int, nbytes: int, stream=None, fancy: bool = False,
                               opts=None) -> None:
        """qs_hip_compress_device_batch_prepare[_opts]: geometry, modes and tables into the workspace (synchronises
        `stream`; not inside a capture); opts as compress_batch_info takes them"""
        if opts is None or fancy:
            self._check(self.lib.qs_hip_compress_device_batch_prepare(self._job_ptrs(jobs), len(jobs), int(bool(fancy)),
                                                                      d_workspace, nbytes, stream))
        else:
            arr, _keep = _named_ptrs(*_COMPRESS_MODES, opts, len(jobs))
            self._check(self.lib.qs_hip_compress_device_batch_prepare_opts(self._job_ptrs(jobs), len(jobs), arr,
                                                                           d_workspace, nbytes, stream))

    def compress_batch(self, jobs, d_pixels, pitch, d_workspace: int, nbytes: int, stream=None) -> None:
        """qs_hip_compress_device_batch: enqueue the compress of every job (one launch per 44 jobs); d_pixels[i] = device
        address of job i's interleaved uint8 pixels, pitch[i] = bytes between its rows; the arrays are job.coef"""
        self._check(self.lib.qs_hip_compress_device_batch(self._job_ptrs(jobs), len(jobs), _c_array(C.c_void_p, d_pixels),
                                                          _c_array(C.c_size_t, pitch), d_workspace, nbytes, stream))

    # -- device entropy coder (a list of device_job() Jobs) -------------------------------
    @staticmethod
    def _opt_ptrs(opts, n):
        """opts: None, or one (restart_interval, restart_in_rows) / None per job -> (the pointer array or None, what it
        points to: keep it alive over the call)"""
        recs = None if opts is None else [None if o is None else EncodeOpts(int(o[0]), int(o[1])) for o in opts]
        return _ptr_array(EncodeOpts, recs, n, "one options entry (or None) per job"), recs

    def encode_batch_info(self, jobs, opts=None):
        """qs_hip_encode_device_batch_info, or _info_opts when opts is given (one (restart_interval, restart_in_rows) or
        None per job); no device needed -> (list of dict(dc_tbl, ac_tbl, blocks_in_mcu, max_segment_bytes), the batch's
        workspace bytes)"""
        per = (EncodeInfo * max(1, len(jobs)))()
        total = C.c_size_t(0)
        if opts is None:
            self._check(self.lib.qs_hip_encode_device_batch_info(self._job_ptrs(jobs), len(jobs), per, C.byref(total)))
        else:
            optr, _keep = self._opt_ptrs(opts, len(jobs))
            self._check(self.lib.qs_hip_encode_device_batch_info_opts(self._job_ptrs(jobs), len(jobs), optr, per,
                                                                      C.byref(total)))
        return [dict(dc_tbl=list(per[i].dc_tbl[:jobs[i].ncomp]), ac_tbl=list(per[i].ac_tbl[:jobs[i].ncomp]),
                     blocks_in_mcu=list(per[i].blocks_in_mcu), max_segment_bytes=int(per[i].max_segment_bytes))
                for i in range(len(jobs))], int(total.value)

    @staticmethod
    def huff_tables(dc=None, ac=None) -> HuffTables:
        """a qs_hip_huff_tables: dc / ac = {table index: (bits[17], huffval)}; a table left out is the standard one"""
        t = HuffTables()
        _fill_huff(dc, t.dc, t.has_dc, (0, 1), "huff_tables")
        _fill_huff(ac, t.ac, t.has_ac, (0, 1), "huff_tables")
        return t

    def encode_batch_prepare(self, jobs, tables, d_workspace: int, nbytes: int, stream=None, opts=None) -> None:
        """qs_hip_encode_device_batch_prepare, or _prepare_opts when opts is given (as encode_batch_info): geometry, code
        tables and restart intervals into the workspace (synchronises `stream`; not inside a capture); tables: None or
        one HuffTables / None per job"""
        ptrs = _ptr_array(HuffTables, tables, len(jobs), "one HuffTables (or None) per job")
        if opts is None:
            self._check(self.lib.qs_hip_encode_device_batch_prepare(self._job_ptrs(jobs), len(jobs), ptrs, d_workspace,
                                                                    nbytes, stream))
        else:
            optr, _keep = self._opt_ptrs(opts, len(jobs))
            self._check(self.lib.qs_hip_encode_device_batch_prepare_opts(self._job_ptrs(jobs), len(jobs), ptrs, optr,
                                                                         d_workspace, nbytes, stream))

    def encode_batch(self, jobs, d_stop, d_out, capacity, d_len: int, d_status: int, d_workspace: int, nbytes: int,
                     stream=None) -> None:
        """qs_hip_encode_device_batch: enqueue the scan coder of every job; d_out[i] = device address of job i's buffer
        of capacity[i] bytes, d_len / d_status = device uint64[njobs] / int32[njobs]"""
        self._check(self.lib.qs_hip_encode_device_batch(self._job_ptrs(jobs), len(jobs), d_stop, _c_array(C.c_void_p, d_out),
                                                        _c_array(C.c_size_t, capacity), d_len, d_status, d_workspace, nbytes,
                                                        stream))

    def encode_batch_histogram(self, jobs, d_stop, d_counts: int, d_status: int, d_workspace: int, nbytes: int,
                               stream=None) -> None:
        """qs_hip_encode_device_batch_histogram: symbol counts uint32[njobs][4][257] (DC 0, DC 1, AC 0, AC 1)"""
        self._check(self.lib.qs_hip_encode_device_batch_histogram(self._job_ptrs(jobs), len(jobs), d_stop, d_counts,
                                                                  d_status, d_workspace, nbytes, stream))

    def huff_optimal_device(self, d_counts: int, ntables: int, d_tables: int, d_status: int, stream=None) -> None:
        """qs_hip_huff_optimal_device: d_counts = device uint32[ntables][257] -> d_tables = device
        qs_hip_huff_table[ntables] (273 bytes each: bits[17], huffval[256]), d_status = device int32[ntables] (0, or 5 for
        a code length above 32); one launch, one wave per table"""
        self._check(self.lib.qs_hip_huff_optimal_device(d_counts, int(ntables), d_tables, d_status, stream))

    def encode_files_scratch_bytes(self, njobs: int) -> int:
        """qs_hip_encode_files_scratch_bytes: what encode_batch_files needs as d_scratch for njobs jobs"""
        return int(self.lib.qs_hip_encode_files_scratch_bytes(int(njobs)))

    @staticmethod
    def encode_frame(head=(None, None), mid=(None, None)) -> EncodeFrame:
        """a qs_hip_encode_frame: head / mid = per variant None or (device address, bytes)"""
        f = EncodeFrame()
        for v in range(2):
            for part, ptr, nb in ((head, f.d_head, f.head_bytes), (mid, f.d_mid, f.mid_bytes)):
                if part[v] is not None:
                    ptr[v], nb[v] = part[v][0] or None, int(part[v][1])
        return f

    @staticmethod
    def _frames(frames, n):
        if len(frames) != n:
            raise ValueError("one EncodeFrame per job")
        return _c_array(EncodeFrame, frames)

    def encode_batch_files(self, jobs, frames, optimize, d_stop, d_out, capacity, d_len: int, d_status: int, d_tables,
                           d_scratch: int, scratch_bytes: int, d_workspace: int, nbytes: int, stream=None) -> None:
        """qs_hip_encode_device_batch_files: enqueue whole files -- head, DHT markers (optimize), mid, segment, EOI -- into
        d_out[i]; frames: None (markers and segment only) or one EncodeFrame per job; d_tables: device
        qs_hip_huff_tables[njobs] or None; the workspace as encode_batch takes it"""
        fr = None if frames is None else self._frames(frames, len(jobs))
        self._check(self.lib.qs_hip_encode_device_batch_files(self._job_ptrs(jobs), len(jobs), fr, 1 if optimize else 0,
                                                              d_stop, _c_array(C.c_void_p, d_out),
                                                              _c_array(C.c_size_t, capacity), d_len, d_status, d_tables,
                                                              d_scratch, scratch_bytes, d_workspace, nbytes, stream))

    # -- progressive files (spectral selection) ---------------------------------------------
    @staticmethod
    def prog_opts(script, restart_interval=0, restart_in_rows=0, component_id=None, refinement=False) -> EncodeProgOpts:
        """a qs_hip_encode_prog_opts: script = [(component indices, Ss, Se, Ah, Al)] (jpeg_file.spectral_script,
        jpeg_file.simple_progression); component_id None: jpeg_set_colorspace's ids; refinement: QS_HIP_PROG_REFINE, without
        which a script with an Ah > 0 scan is refused"""
        script = list(script)
        arr = (EncodeScan * max(1, len(script)))()
        for r, (comps, ss, se, ah, al) in zip(arr, script):
            comps = list(comps)
            r.ncomp = len(comps)
            for k, c in enumerate(comps[:4]):
                r.comp[k] = int(c)
            r.Ss, r.Se, r.Ah, r.Al = int(ss), int(se), int(ah), int(al)
        o = EncodeProgOpts(C.cast(arr, C.POINTER(EncodeScan)), len(script), int(restart_interval), int(restart_in_rows))
        for k, v in enumerate(component_id or ()):
            o.component_id[k] = int(v)
        o.flags = PROG_REFINE if refinement else 0
        o._scans = arr                                                  # (kept alive with the record)
        return o

    @staticmethod
    def _prog_opt_ptrs(opts, n):
        return _ptr_array(EncodeProgOpts, opts, n, "one EncodeProgOpts per job")

    def encode_progressive_info(self, jobs, opts):
        """qs_hip_encode_progressive_device_batch_info; no device needed -> (list of dict(nscans, mcus, interval,
        max_body_bytes), workspace bytes, scratch bytes)"""
        per = (EncodeProgInfo * max(1, len(jobs)))()
        ws, sc = C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.qs_hip_encode_progressive_device_batch_info(self._job_ptrs(jobs), len(jobs),
                                                                         self._prog_opt_ptrs(opts, len(jobs)), per,
                                                                         C.byref(ws), C.byref(sc)))
        return [dict(nscans=int(p.nscans), mcus=list(p.mcus[:p.nscans]), interval=list(p.interval[:p.nscans]),
                     max_body_bytes=int(p.max_body_bytes)) for p in per[:len(jobs)]], int(ws.value), int(sc.value)

    def encode_progressive_prepare(self, jobs, opts, d_workspace: int, nbytes: int, stream=None) -> None:
        """qs_hip_encode_progressive_device_batch_prepare: the scan jobs and their DRI / SOS bytes into the workspace
        (synchronises `stream`; not inside a capture)"""
        self._check(self.lib.qs_hip_encode_progressive_device_batch_prepare(self._job_ptrs(jobs), len(jobs),
                                                                            self._prog_opt_ptrs(opts, len(jobs)),
                                                                            d_workspace, nbytes, stream))

    def encode_progressive_files(self, jobs, frames, d_stop, d_out, capacity, d_len: int, d_status: int, d_scratch: int,
                                 scratch_bytes: int, d_workspace: int, nbytes: int, stream=None) -> None:
        """qs_hip_encode_progressive_device_batch_files: enqueue whole progressive files into d_out[i]; frames: one
        EncodeFrame per job (its heads: SOI .. SOF2)"""
        self._check(self.lib.qs_hip_encode_progressive_device_batch_files(self._job_ptrs(jobs), len(jobs),
                                                                          self._frames(frames, len(jobs)), d_stop,
                                                                          _c_array(C.c_void_p, d_out),
                                                                          _c_array(C.c_size_t, capacity), d_len, d_status,
                                                                          d_scratch, scratch_bytes, d_workspace, nbytes, stream))

    # -- device scan reader (a list of device_job() Jobs over the arrays to fill) ---------
    @staticmethod
    def read_opts(dc=None, ac=None, dc_tbl=(), ac_tbl=(), restart_interval=0) -> ReadOpts:
        """a qs_hip_read_opts: dc / ac = {DHT id 0..3: (bits[17], huffval)} (a table left out is the standard one),
        dc_tbl / ac_tbl = Td / Ta of each component, restart_interval = the DRI value"""
        o = ReadOpts()
        _fill_huff(dc, o.dc, o.has_dc, (0, 1, 2, 3), "read_opts")
        _fill_huff(ac, o.ac, o.has_ac, (0, 1, 2, 3), "read_opts")
        for ci, (td, ta) in enumerate(zip(dc_tbl, ac_tbl)):
            o.dc_tbl[ci], o.ac_tbl[ci] = int(td), int(ta)
        o.restart_interval = int(restart_interval)
        return o

    @staticmethod
    def _read_opt_ptrs(opts, n):
        return _ptr_array(ReadOpts, opts, n, "one ReadOpts per job")

    def read_batch_info(self, jobs, opts, split=False):
        """qs_hip_read_device_batch_info (no device needed) -> (list of dict(blocks_in_mcu, mcus, intervals,
        blocks_per_interval), the batch's workspace bytes).  split: qs_hip_read_split_device_batch_info, the split
        route (no interval cap; the dicts also hold max_segments); its workspace is another one"""
        info = ReadSplitInfo if split else ReadInfo
        call = self.lib.qs_hip_read_split_device_batch_info if split else self.lib.qs_hip_read_device_batch_info
        per = (info * max(1, len(jobs)))()
        total = C.c_size_t(0)
        self._check(call(self._job_ptrs(jobs), len(jobs), self._read_opt_ptrs(opts, len(jobs)), per, C.byref(total)))
        return [_info_dict(p) for p in per[:len(jobs)]], int(total.value)

    def read_batch_prepare(self, jobs, opts, d_workspace: int, nbytes: int, stream=None, split=False) -> None:
        """qs_hip_read_device_batch_prepare (split: qs_hip_read_split_device_batch_prepare): geometry and derived code
        tables into the workspace (synchronises `stream`; not inside a capture)"""
        call = self.lib.qs_hip_read_split_device_batch_prepare if split else self.lib.qs_hip_read_device_batch_prepare
        self._check(call(self._job_ptrs(jobs), len(jobs), self._read_opt_ptrs(opts, len(jobs)), d_workspace, nbytes, stream))

    def read_batch(self, jobs, d_scan, scan_bytes, d_status: int, d_workspace: int, nbytes: int, stream=None,
                   split=False) -> None:
        """qs_hip_read_device_batch (split: qs_hip_read_split_device_batch): enqueue the scan reader of every job;
        d_scan[i] = device address of job i's bytes behind the SOS header, scan_bytes[i] = how many may be read,
        d_status = device int32[njobs]"""
        scans, lens = _c_array(C.c_void_p, d_scan), _c_array(C.c_uint64, [int(v) for v in scan_bytes])
        call = self.lib.qs_hip_read_split_device_batch if split else self.lib.qs_hip_read_device_batch
        self._check(call(self._job_ptrs(jobs), len(jobs), scans, lens, d_status, d_workspace, nbytes, stream))

    # -- its progressive route (whole SOF2 files) ----------------------------------------
    @staticmethod
    def read_prog_opts(scans) -> ReadProgOpts:
        """a qs_hip_read_prog_opts from jpeg_file.parse_progressive(...)["scans"]: per scan dict(comps, ss, se, ah, al,
        dc_tbl, ac_tbl, dc, ac ({DHT id: (bits[17], huffval)} in effect), restart_interval, offset)"""
        scans = list(scans)
        arr = (ReadProgScan * max(1, len(scans)))()
        for r, s in zip(arr, scans):
            comps = list(s["comps"])
            r.scan.ncomp = len(comps)
            for k, c in enumerate(comps[:4]):
                r.scan.comp[k] = int(c)
            r.scan.Ss, r.scan.Se, r.scan.Ah, r.scan.Al = int(s["ss"]), int(s["se"]), int(s["ah"]), int(s["al"])
            for k, (td, ta) in enumerate(list(zip(s["dc_tbl"], s["ac_tbl"]))[:4]):
                r.dc_tbl[k], r.ac_tbl[k] = int(td), int(ta)
            _fill_huff(s.get("dc"), r.dc, r.has_dc, (0, 1, 2, 3), "read_prog_opts")
            _fill_huff(s.get("ac"), r.ac, r.has_ac, (0, 1, 2, 3), "read_prog_opts")
            r.restart_interval = int(s["restart_interval"])
            r.offset = int(s["offset"])
        o = ReadProgOpts(C.cast(arr, C.POINTER(ReadProgScan)), len(scans))
        o._scans = arr                                                  # (kept alive with the record)
        return o

    @staticmethod
    def _read_prog_opt_ptrs(opts, n):
        return _ptr_array(ReadProgOpts, opts, n, "one ReadProgOpts per job")

    def read_prog_batch_info(self, jobs, opts):
        """qs_hip_read_prog_device_batch_info (no device needed) -> (list of dict(nscans, levels, mcus, intervals), the
        batch's workspace bytes)"""
        per = (ReadProgInfo * max(1, len(jobs)))()
        total = C.c_size_t(0)
        self._check(self.lib.qs_hip_read_prog_device_batch_info(self._job_ptrs(jobs), len(jobs),
                                                                self._read_prog_opt_ptrs(opts, len(jobs)), per,
                                                                C.byref(total)))
        return [dict(nscans=int(p.nscans), levels=int(p.levels), mcus=list(p.mcus[:p.nscans]),
                     intervals=list(p.intervals[:p.nscans])) for p in per[:len(jobs)]], int(total.value)

    def read_prog_batch_prepare(self, jobs, opts, d_workspace: int, nbytes: int, stream=None) -> None:
        """qs_hip_read_prog_device_batch_prepare: the (job, scan) pairs' descriptors and the level lists into the
        workspace (synchronises `stream`; not inside a capture)"""
        self._check(self.lib.qs_hip_read_prog_device_batch_prepare(self._job_ptrs(jobs), len(jobs),
                                                                   self._read_prog_opt_ptrs(opts, len(jobs)), d_workspace,
                                                                   nbytes, stream))

    def read_prog_batch(self, jobs, d_file, file_bytes, d_status: int, d_workspace: int, nbytes: int, stream=None) -> None:
        """qs_hip_read_prog_device_batch: enqueue the progressive reader of every job; d_file[i] = device address of job
        i's whole file, file_bytes[i] = how many bytes may be read there, d_status = device int32[njobs]"""
        files, lens = _c_array(C.c_void_p, d_file), _c_array(C.c_uint64, [int(v) for v in file_bytes])
        self._check(self.lib.qs_hip_read_prog_device_batch(self._job_ptrs(jobs), len(jobs), files, lens, d_status,
                                                           d_workspace, nbytes, stream))

    def huff_optimal(self, freq):
        """qs_hip_huff_optimal (host only): symbol counts (256 or 257) -> (bits[17], huffval) as libjpeg's
        optimize_coding makes them"""
        f = (C.c_uint32 * 257)(*([int(v) for v in list(freq)[:256]] + [1]))
        bits, vals = (C.c_uint8 * 17)(), (C.c_uint8 * 256)()
        self._check(self.lib.qs_hip_huff_optimal(f, bits, vals))
        return list(bits), list(vals)[:sum(bits)]

    def huff_standard(self, is_ac: int, tbl: int):
        """qs_hip_huff_standard (host only): the table of JPEG Annex K.3 -> (bits[17], huffval)"""
        bits, vals = (C.c_uint8 * 17)(), (C.c_uint8 * 256)()
        self._check(self.lib.qs_hip_huff_standard(int(is_ac), int(tbl), bits, vals))
        return list(bits), list(vals)[:sum(bits)]

    # -- plane layer (device pointers as ints, stream as int or None) ----------
    def idct_plane(self, d_consts, d_coef, d_plane, wblk, hblk, first, rep_top, rep_bot, d_status, stream=None):
        self._check(self.lib.qs_hip_idct_plane(d_consts, d_coef, d_plane, wblk, hblk, int(first),
                                               int(rep_top), int(rep_bot), d_status, stream))

    def smooth_plane(self, d_consts, d_coef, d_plane, wblk, hblk, flags, luma=1, final_clamp=0, stream=None):
        self._check(self.lib.qs_hip_smooth_plane(d_consts, d_coef, d_plane, wblk, hblk, flags,
                                                 int(luma), int(final_clamp), stream))

    def smooth_plane_next(self, d_consts, d_coef, d_plane, d_plane_next, wblk, hblk, flags, luma=1, final_clamp=0,
                          rep_top=1, rep_bot=1, stream=None):
        """pass B that also writes the NEXT iteration's pixel plane (fused pass A) into d_plane_next"""
        self._check(self.lib.qs_hip_smooth_plane_next(d_consts, d_coef, d_plane, d_plane_next, wblk, hblk, flags,
                                                      int(luma), int(final_clamp), int(rep_top), int(rep_bot), stream))

    @staticmethod
    def plane_refs(planes):
        """[(d_consts, d_coef, d_plane, d_status, wblk, hblk, luma[, band[, d_plane_next]])] -> PlaneRefs for the
        *_planes calls; band: bit 0 / bit 1 = the top / bottom apron row is a halo row (a band of a sharded plane), bit 2 =
        QS_HIP_PLANE_DEFER (deferred dequantisation: the first pass A and the first smoothing launch only, see the header);
        d_plane_next: the plane the smoothing launch writes the next iteration's pixels into (None: none) -- these go
        into the parallel array of qs_hip_smooth_planes_next, the struct itself has no such field"""
        arr = (PlaneRef * len(planes))()
        nxt = (C.c_void_p * len(planes))()
        any_next = False
        for i, (r, p) in enumerate(zip(arr, planes)):
            cst, coef, plane, status, wb, hb, luma = p[:7]
            r.d_consts, r.d_coef, r.d_plane, r.d_status = cst, coef, plane, status
            r.wblk, r.hblk, r.luma = wb, hb, int(luma)
            r.band = int(p[7]) if len(p) > 7 else 0
            nxt[i] = p[8] if len(p) > 8 else None
            any_next = any_next or bool(nxt[i])
        return PlaneRefs(arr, nxt if any_next else None)

    def idct_planes(self, refs, first, stream=None):
        self._check(self.lib.qs_hip_idct_planes(refs.arr, len(refs), int(first), stream))

    def smooth_planes(self, refs, flags, final_clamp=0, stream=None):
        if refs.next is not None:
            self._check(self.lib.qs_hip_smooth_planes_next(refs.arr, refs.next, len(refs), flags, int(final_clamp), stream))
        else:
            self._check(self.lib.qs_hip_smooth_planes(refs.arr, len(refs), flags, int(final_clamp), stream))

    def smooth_rows(self, d_consts, d_coef, d_plane, wblk, hblk, row0, row1, flags, luma=1, final_clamp=0, stream=None):
        self._check(self.lib.qs_hip_smooth_rows(d_consts, d_coef, d_plane, wblk, hblk, row0, row1, flags,
                                                int(luma), int(final_clamp), stream))

    def joint_plane(self, d_consts, d_coef, d_plane, d_lowres, wblk, hblk, rebalance=0, final_clamp=0, stream=None):
        self._check(self.lib.qs_hip_joint_plane(d_consts, d_coef, d_plane, d_lowres, wblk, hblk,
                                                int(rebalance), int(final_clamp), stream))

    def lowq_plane(self, d_consts, d_coef, d_plane, wblk, hblk, rebalance=1, final_clamp=0, stream=None):
        self._check(self.lib.qs_hip_lowq_plane(d_consts, d_coef, d_plane, wblk, hblk, int(rebalance), int(final_clamp), stream))

    def downsample_plane(self, d_luma, ywblk, yhblk, d_lowres, lwblk, lhblk, ws, hs, stream=None):
        self._check(self.lib.qs_hip_downsample_plane(d_luma, ywblk, yhblk, d_lowres, lwblk, lhblk, ws, hs, stream))

    def upsample_pitch(self, image_width, ws):
        return self.lib.qs_hip_upsample_pitch(image_width, ws)

    def upsample_rows(self, d_chroma, d_lowres, cwblk, d_luma, ywblk, yhblk, d_pixels, pitch, w1, h1, first_rows, ws, hs, stream=None):
        self._check(self.lib.qs_hip_upsample_rows(d_chroma, d_lowres, cwblk, d_luma, ywblk, yhblk, d_pixels, pitch,
                                                  w1, h1, first_rows, ws, hs, stream))

    def fdct_plane(self, d_pixels, pitch, d_coef, wblk, hblk, stream=None):
        self._check(self.lib.qs_hip_fdct_plane(d_pixels, pitch, d_coef, wblk, hblk, stream))

    def clamp_plane(self, d_coef, wblk, hblk, stream=None):
        self._check(self.lib.qs_hip_clamp_plane(d_coef, wblk, hblk, stream))

    def dequant_plane(self, d_consts, d_coef, wblk, hblk, stream=None):
        self._check(self.lib.qs_hip_dequant_plane(d_consts, d_coef, wblk, hblk, stream))
