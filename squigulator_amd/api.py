"""ctypes binding of the C ABI in include/sqg.h, include/sqg_chunks.h, include/sqg_targets.h, include/sqg_segments.h, include/sqg_sites.h, include/sqg_events.h, include/sqg_pileup.h, include/sqg_detect.h, include/sqg_align.h, include/sqg_collapse.h and include/sqg_scale.h (squigulator_amd/csrc/libsqg_hip.so).

This is plumbing for tests and bench.py; the product is the shared library.  There is NO CPU
fallback: if the HIP library is missing or no GPU is usable, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build
from . import profiles as P

ABI_VERSION = 2
MODE_EXACT = 0
MODE_CERTIFIED = 1

_ERRORS = {-1: "SQG_EINVAL", -2: "SQG_ENOMEM", -3: "SQG_EDEVICE", -4: "SQG_ESEQUENCE",
           -5: "SQG_ENODEVICE", -6: "SQG_EOVERFLOW", -7: "SQG_EIO"}


class SqgError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where}: {_ERRORS.get(code, code)} {detail}".strip())


class CProfile(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "digitisation", "sample_rate", "bps", "range", "offset_mean", "offset_std",
        "median_before_mean", "median_before_std", "dwell_mean", "dwell_std")]


class CKmer(C.Structure):
    _fields_ = [("level_mean", C.c_float), ("level_stdv", C.c_float)]


class CCfg(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("profile", CProfile), ("flags", C.c_uint32),
                ("amp_noise", C.c_float), ("kmer_size", C.c_uint32), ("model", C.POINTER(CKmer)),
                ("seed", C.c_int64), ("num_workers", C.c_int32), ("worker_lo", C.c_int32),
                ("worker_hi", C.c_int32), ("device", C.c_int32), ("mode", C.c_uint32)]


class CResult(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("n_events", C.c_int64), ("n_samples", C.c_int64),
                ("n_bases", C.c_int64), ("sig_off", C.POINTER(C.c_int64)), ("ev_off", C.POINTER(C.c_int64)),
                ("offset", C.POINTER(C.c_double)), ("median_before", C.POINTER(C.c_double)),
                ("d_signal", C.c_void_p), ("d_dwell", C.c_void_p)]


class CTiming(C.Structure):
    _fields_ = [("dwell_ms", C.c_float), ("events_ms", C.c_float), ("samples_ms", C.c_float),
                ("lean_ms", C.c_float), ("total_ms", C.c_float), ("fallback_samples", C.c_int64),
                ("carried_first_pass", C.c_int32), ("first_pass_ran_ahead", C.c_int32)]


class CSvb(C.Structure):
    _fields_ = [("n_bytes", C.c_int64), ("svb_off", C.POINTER(C.c_int64)), ("d_svb", C.c_void_p)]


class CGenome(C.Structure):
    _fields_ = [("n_contigs", C.c_int32), ("seqs", C.c_void_p), ("contig_off", C.POINTER(C.c_int64)),
                ("rlen", C.c_int32), ("mode", C.c_uint32), ("n_trans", C.c_int32),
                ("trans_csum", C.POINTER(C.c_float)), ("trans_idx", C.POINTER(C.c_int32))]


class CSample(C.Structure):
    _fields_ = [("ref_idx", C.POINTER(C.c_int32)), ("ref_len", C.POINTER(C.c_int32)), ("ref_pos", C.POINTER(C.c_int32)),
                ("rlen", C.POINTER(C.c_int32)), ("strand", C.POINTER(C.c_char)), ("seq_off", C.POINTER(C.c_int64))]


SAMPLE_DNA, SAMPLE_RNA, SAMPLE_CDNA, SAMPLE_TRUNC, SAMPLE_FULL = 0, 1, 2, 4, 8
BLOW5_STORED = 0x10000          # include/sqg.h SQG_BLOW5_STORED (flags of sqg_blow5_open)
BLOW5_HUFFMAN = 0x20000         # include/sqg.h SQG_BLOW5_HUFFMAN (flags of sqg_blow5_open and sqg_batch_blow5_records)

EXPORTS = ("sqg_create", "sqg_destroy", "sqg_last_error", "sqg_strerror", "sqg_device_count",
           "sqg_batch_stage", "sqg_batch_run", "sqg_batch_wait", "sqg_fetch_signal", "sqg_fetch_dwell",
           "sqg_batch_free", "sqg_get_timing", "sqg_set_phase_timing", "sqg_submit", "sqg_worker_of", "sqg_probe_store_bandwidth", "sqg_probe_lds_order",
           "sqg_batch_compress", "sqg_fetch_svb", "sqg_genome_load", "sqg_batch_sample", "sqg_fetch_reads",
           "sqg_host_alloc", "sqg_host_free", "sqg_set_range_mode", "sqg_skip_reads", "sqg_batch_sample_range",
           "sqg_batch_run_begin", "sqg_batch_run_end", "sqg_genome_load_device",
           "sqg_blow5_open", "sqg_blow5_write", "sqg_blow5_write_batch", "sqg_blow5_close", "sqg_blow5_last_error", "sqg_batch_blow5_records",
           "sqg_genome_set_meth", "sqg_build_info", "sqg_set_stage_threads")

# Environment knobs only the development build of the library reads (csrc/h_common.h: SQG_DEV_ENV; tools/README.md).  The release
# library ignores them, so a process that sets one -- a test forcing a code path, an A/B script -- gets libsqg_hip_dev.so.
DEV_KNOBS = ("SQG_EVENTS_WIDE_MAX", "SQG_TEST_ORDER_FAULT", "SQG_ABL_NOFIX", "SQG_SAMPLER_SERIAL", "SQG_PART_CLAIMS",
             "SQG_TEST_DELTA_X", "SQG_TEST_ROW_TURNS", "SQG_PART_WG_EVENTS", "SQG_SPLIT_CHAINS", "SQG_NO_PART",
             "SQG_PART_SLICE", "SQG_TEST_NO_LEAN", "SQG_STAGE_THREADS", "SQG_NO_PRECOUNT", "SQG_NO_DRAW_AHEAD",
             "SQG_NO_PLACE", "SQG_TEST_B5_MAXBITS", "SQG_TEST_CHUNK_GENERIC", "SQG_TEST_SEG_SPS", "SQG_TEST_SCALE_GRID", "SQG_TEST_CALL_GRID",
             "SQG_TEST_MAP_TILES")

# include/sqg_chunks.h: bound by load_library only when the library has them (the CPU backend does not)
EXPORTS_CHUNKS = ("sqg_chunk_plan", "sqg_batch_chunks")
CHUNK_F16, CHUNK_F32 = 0, 1
CHUNK_MEDMAD, CHUNK_PA = 0, 1


class CChunkCfg(C.Structure):
    _fields_ = [("chunk_len", C.c_int32), ("stride", C.c_int32), ("max_label", C.c_int32), ("dtype", C.c_uint32), ("norm", C.c_uint32)]


class CChunkOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("signal", "labels", "label_len", "chunk_read", "chunk_start", "med2", "mad4")]


# include/sqg_targets.h: bound the same way
EXPORTS_TARGETS = ["sqg_batch_chunk_targets"]


class CChunkTargets(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("clean", "clean_raw", "moves", "kmer", "med2", "mad4")]


# include/sqg_segments.h: bound the same way
EXPORTS_SEGMENTS = ("sqg_batch_segments", "sqg_chunk_plan_trimmed", "sqg_batch_chunks_trimmed", "sqg_batch_chunk_targets_trimmed")


class CSegments(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("seg", "shift")]


# include/sqg_sites.h: bound the same way
EXPORTS_SITES = ("sqg_site_plan", "sqg_batch_sites")
SITE_OUTPUTS = ("signal", "label", "site_read", "site_pos", "win_start", "context", "ctx_start", "med2", "mad4")


class CSiteCfg(C.Structure):
    _fields_ = [("win_len", C.c_int32), ("before", C.c_int32), ("focus", C.c_int32), ("ctx_len", C.c_int32), ("ctx_before", C.c_int32),
                ("dtype", C.c_uint32), ("norm", C.c_uint32)]


class CSiteOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SITE_OUTPUTS]


# include/sqg_events.h: bound the same way
EXPORTS_EVENTS = ("sqg_batch_events",)
EVENT_OUTPUTS = ("ev_read", "ev_start", "ev_len", "sum", "sumsq", "vmin", "vmax", "kmer", "level_raw", "seg", "mean", "sd", "med2", "mad4")


class CEventCfg(C.Structure):
    _fields_ = [("norm", C.c_uint32), ("trim", C.c_int32)]


class CEventOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in EVENT_OUTPUTS]


# include/sqg_pileup.h: bound the same way
EXPORTS_PILEUP = ("sqg_batch_pileup",)
PILEUP_OUTPUTS = ("n", "dwell", "dwell_sq", "mean_sum", "mean_sq", "sd_sum")
PILEUP_BY_REF, PILEUP_BY_KMER = 0, 1
PILEUP_SPLIT_STRAND, PILEUP_SPLIT_METH = 1, 2


class CPileupCfg(C.Structure):
    _fields_ = [("by", C.c_uint32), ("split", C.c_uint32), ("norm", C.c_uint32), ("trim", C.c_int32), ("segs", C.c_uint32),
                ("lo", C.c_int64), ("hi", C.c_int64)]


class COrigin(C.Structure):
    _fields_ = [("key0", C.POINTER(C.c_int64)), ("step", C.POINTER(C.c_int8))]


class CPileupOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PILEUP_OUTPUTS]


class CPileupStat(C.Structure):
    _fields_ = [("counted", C.c_int64), ("outside", C.c_int64)]


# include/sqg_detect.h: bound the same way
EXPORTS_DETECT = ("sqg_detect_plan", "sqg_batch_detect")
DETECT_OUTPUTS = ("dt_read", "dt_start", "dt_len", "sum", "sumsq", "vmin", "vmax", "mean", "sd", "true_ev", "med2", "mad4")
DETECT_PRESETS = {"dna": (3, 6, 1.4, 9.0, 0.2), "rna": (7, 14, 2.5, 9.0, 1.0)}        # SQG_DETECT_DNA, SQG_DETECT_RNA


class CDetectCfg(C.Structure):
    _fields_ = [("w_short", C.c_int32), ("w_long", C.c_int32), ("thr_short", C.c_double), ("thr_long", C.c_double), ("peak_height", C.c_double),
                ("norm", C.c_uint32), ("trim", C.c_int32)]


class CDetectOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in DETECT_OUTPUTS]


# include/sqg_align.h: bound the same way
EXPORTS_ALIGN = ("sqg_batch_align",)
ALIGN_OUTPUTS = ("al_ev", "al_cost", "al_edge")
ALIGN_DEFAULT = (4096, 4096, 65536)                         # SQG_ALIGN_DEFAULT
ALIGN_BAND = 64


class CAlignCfg(C.Structure):
    _fields_ = [("stay_pen", C.c_int32), ("skip_pen", C.c_int32), ("cost_cap", C.c_int32)]


class CAlignIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("sum", "len")]


class CAlignOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ALIGN_OUTPUTS]


# include/sqg_scale.h: bound the same way
EXPORTS_SCALE = ("sqg_batch_scale", "sqg_batch_align_scaled")
SCALE_MOMENTS, SCALE_FIT = 0, 1
SCALE_INPUTS = ("sum", "len", "ev")
SCALE_OUTPUTS = ("n", "nx", "sy", "syy", "sx", "sxx", "sxy", "gain", "shift", "rd_dropped")


class CScaleCfg(C.Structure):
    _fields_ = [("mode", C.c_uint32)]


class CScaleIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SCALE_INPUTS]


class CScaleOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SCALE_OUTPUTS]


class CAlignScale(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("gain", "shift")]


# include/sqg_call.h: bound the same way
EXPORTS_CALL = ("sqg_call_plan", "sqg_batch_call")
CALL_NEIGH_READ, CALL_NEIGH_SAME = 0, 1
CALL_DEFAULT = (CALL_NEIGH_SAME, 256 * 50, 256 * 2, 1)         # SQG_CALL_DEFAULT
CALL_OUTPUTS = ("site_read", "site_pos", "label", "site_key", "n_obs", "nll_c", "nll_m", "llr", "call")
CALL_FREQ = ("cov", "truth", "called", "meth")


class CCallCfg(C.Structure):
    _fields_ = [("neigh", C.c_uint32), ("term_cap", C.c_int32), ("llr_min", C.c_int32), ("min_obs", C.c_int32)]


class CCallIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("sum", "len64", "len32")]


class CCallModel(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w", "c")]


class CCallOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in CALL_OUTPUTS]


class CCallFreq(C.Structure):
    _fields_ = [("lo", C.c_int64), ("hi", C.c_int64)] + [(n, C.c_void_p) for n in CALL_FREQ]


class CCallStat(C.Structure):
    _fields_ = [("sites", C.c_int64), ("outside", C.c_int64), ("called", C.c_int64), ("agree", C.c_int64)]


# include/sqg_map.h: bound the same way; sqg_map_track takes no batch, and its window by value
EXPORTS_MAP = ("sqg_map_track", "sqg_batch_map")
MAP_OUTPUTS = ("map_cost", "map_step", "map_key0", "map_key1", "map_cost_other")
MAP_CFG = ("stay_pen", "skip_pen", "cost_cap", "row_first", "row_count", "strands")
MAP_DEFAULT = (min(ALIGN_DEFAULT[0], 1 << 17), min(ALIGN_DEFAULT[1], 1 << 17), min(ALIGN_DEFAULT[2], 1 << 17), 0, 256, 3)     # SQG_MAP_DEFAULT
MAP_NONE = -(1 << 31)                                       # SQG_MAP_NONE
MAP_MAX_WINDOW, MAP_MAX_ROWS = 1 << 24, 4096


class CMapCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in MAP_CFG[:5]] + [("strands", C.c_uint32)]


class CMapTrack(C.Structure):
    _fields_ = [("lo", C.c_int64), ("hi", C.c_int64), ("fwd", C.c_void_p), ("rev", C.c_void_p)]


class CMapOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MAP_OUTPUTS]


class MapTrack:
    """What SignalGenerator.new_map_track() returns and Batch.map() takes: the window [lo, hi) and its levels on either strand, int32 torch
    tensors [hi - lo] on the context's device (include/sqg_map.h says what they hold); one not asked for is None"""

    def __init__(self, lo, hi, fwd, rev):
        self.lo, self.hi, self.fwd, self.rev = int(lo), int(hi), fwd, rev


# include/sqg_collapse.h: bound the same way
EXPORTS_COLLAPSE = ("sqg_batch_collapse", "sqg_batch_pileup_rows")
COLLAPSE_INPUTS = ("ev", "sum", "sumsq", "len")
COLLAPSE_OUTPUTS = ("ob_rows", "ob_len", "ob_sum", "ob_sumsq", "mean", "sd", "rd_dropped")


class CCollapseCfg(C.Structure):
    _fields_ = [("norm", C.c_uint32), ("trim", C.c_int32)]


class CCollapseIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in COLLAPSE_INPUTS]


class CCollapseOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in COLLAPSE_OUTPUTS]


class CPileupRowsStat(C.Structure):
    _fields_ = [("counted", C.c_int64), ("outside", C.c_int64), ("unseen", C.c_int64), ("dropped", C.c_int64)]


class Pileup:
    """What SignalGenerator.new_pileup() returns: the cfg of a pileup and its sums, torch tensors [planes, hi - lo] on the context's device
    that Batch.pileup() adds to (include/sqg_pileup.h says what they hold); those not asked for are None"""

    def __init__(self, cfg, planes, **kw):
        self.cfg, self.planes = cfg, planes
        self.__dict__.update(kw)


class CallFreq:
    """What SignalGenerator.new_call_freq() returns: the key window [lo, hi) and the four sums Batch.call(freq=...) adds to, torch tensors
    [hi - lo] on the context's device (uint32 bit patterns in int32 tensors; include/sqg_call.h says what they hold)"""

    def __init__(self, lo, hi, **kw):
        self.lo, self.hi = lo, hi
        self.__dict__.update(kw)


class Chunks:
    """What Batch.chunks() returns: torch tensors on the context's device (include/sqg_chunks.h says what they hold)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

# the consumer calls by header: name -> what its arguments behind (context, batch) point to
_PLAN = (C.c_int64, C.c_int64)
_CONSUMER_EXPORTS = (
    (EXPORTS_CHUNKS, {"sqg_chunk_plan": (CChunkCfg,) + _PLAN, "sqg_batch_chunks": (CChunkCfg, CChunkOut)}),
    (EXPORTS_TARGETS, {"sqg_batch_chunk_targets": (CChunkCfg, CChunkTargets)}),
    (EXPORTS_SEGMENTS, {"sqg_batch_segments": (CSegments,), "sqg_chunk_plan_trimmed": (CChunkCfg,) + _PLAN,
                        "sqg_batch_chunks_trimmed": (CChunkCfg, CChunkOut), "sqg_batch_chunk_targets_trimmed": (CChunkCfg, CChunkTargets)}),
    (EXPORTS_SITES, {"sqg_site_plan": (CSiteCfg,) + _PLAN, "sqg_batch_sites": (CSiteCfg, CSiteOut)}),
    (EXPORTS_EVENTS, {"sqg_batch_events": (CEventCfg, CEventOut)}),
    (EXPORTS_PILEUP, {"sqg_batch_pileup": (CPileupCfg, COrigin, CPileupOut, CPileupStat)}),
    (EXPORTS_DETECT, {"sqg_detect_plan": (CDetectCfg,) + _PLAN, "sqg_batch_detect": (CDetectCfg, CDetectOut)}),
    (EXPORTS_ALIGN, {"sqg_batch_align": (CAlignCfg, C.c_int64, CAlignIn, CAlignOut)}),
    (EXPORTS_CALL, {"sqg_call_plan": _PLAN,
                    "sqg_batch_call": (CCallCfg, CCallIn, CCallModel, CAlignScale, COrigin, CCallOut, CCallFreq, CCallStat)}),
    (EXPORTS_MAP, {"sqg_batch_map": (CMapCfg, C.c_int64, CAlignIn, CAlignScale, CMapTrack, CMapOut)}),      # (sqg_map_track: _MAP_TRACK_ARGS)
    (EXPORTS_SCALE, {"sqg_batch_scale": (CScaleCfg, C.c_int64, CScaleIn, CScaleOut),
                     "sqg_batch_align_scaled": (CAlignCfg, C.c_int64, CAlignIn, CAlignScale, CAlignOut)}),
    (EXPORTS_COLLAPSE, {"sqg_batch_collapse": (CCollapseCfg, C.c_int64, CCollapseIn, CCollapseOut),
                        "sqg_batch_pileup_rows": (CPileupCfg, COrigin, C.c_int64, CCollapseIn, CPileupOut, CPileupRowsStat)}),
)

# sqg_map_track is the one consumer call that takes no batch and two arguments by value: (ctx, lo, hi, levels, fwd, rev), bound on its own
_MAP_TRACK_ARGS = (C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)

_ENUMS = {"dtype": {"f16": CHUNK_F16, "f32": CHUNK_F32}, "norm": {"medmad": CHUNK_MEDMAD, "pa": CHUNK_PA},
          "by": {"ref": PILEUP_BY_REF, "kmer": PILEUP_BY_KMER}, "mode": {"moments": SCALE_MOMENTS, "fit": SCALE_FIT},
          "neigh": {"read": CALL_NEIGH_READ, "same": CALL_NEIGH_SAME}}


def _enum(who, **given):
    """the C values of dtype= / norm= / by= given by name or by number, in the order given; SqgError naming them all when one is unknown"""
    vals = [_ENUMS[k].get(v, v) for k, v in given.items()]
    if not all(isinstance(v, int) for v in vals):
        raise SqgError(-1, who, f"unknown {' / '.join(given)} {' / '.join(repr(v) for v in given.values())}")
    return [v & 0xffffffff for v in vals]


def _need(L, export, header, who):
    """the guard of a call the CPU backend lacks"""
    if not hasattr(L, export):
        raise SqgError(-1, who, f"this backend has no {export} (include/{header})")


def _want(outputs, names, who):
    """the set of output names asked for (None: all of them)"""
    want = set(names if outputs is None else outputs)
    if want - set(names):
        raise SqgError(-1, who, f"unknown outputs {sorted(want - set(names))}")
    return want


_len = len                  # (Batch.align() takes the header's name `len` as a parameter)


def _ptrs(struct, tensors):
    """the C struct of device addresses: NULL for an output not wanted or empty"""
    return struct(*(t.data_ptr() if t is not None and t.numel() else None for t in tensors))


_libs = {}                  # absolute path -> loaded library
LOADED_PATH = None          # the library the last load_library() call opened (bench.py prints it with its hash)


def dev_knobs_set() -> list:
    return [k for k in DEV_KNOBS if k in os.environ]


def default_library_path() -> str:
    """SQG_LIB (A/B testing of kernel build variants), else the development build if the environment holds one of its knobs,
    else the release library"""
    return os.environ.get("SQG_LIB") or (_build.LIB_DEV if dev_knobs_set() else _build.LIB)


def build_info(L) -> dict:
    """sqg_build_info() as a dict: {"source_hash": ..., "dev": "0"|"1"}"""
    return dict(kv.split("=", 1) for kv in L.sqg_build_info().decode().split(";") if "=" in kv)


def load_library(path: str | None = None):
    """dlopen the HIP library; raises if it has not been built (no fallback)."""
    path = os.path.abspath(path or default_library_path())
    global LOADED_PATH
    if path in _libs:
        LOADED_PATH = path
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -m squigulator_amd.build` "
                           "(there is no CPU fallback for the signal path)")
    L = C.CDLL(path)
    LOADED_PATH = path
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.sqg_create.restype = C.c_int
    L.sqg_create.argtypes = [C.POINTER(CCfg), C.POINTER(vp)]
    L.sqg_destroy.restype = None
    L.sqg_destroy.argtypes = [vp]
    L.sqg_last_error.restype = C.c_char_p
    L.sqg_last_error.argtypes = [vp]
    L.sqg_strerror.restype = C.c_char_p
    L.sqg_strerror.argtypes = [C.c_int]
    L.sqg_device_count.restype = C.c_int
    L.sqg_batch_stage.restype = C.c_int
    L.sqg_batch_stage.argtypes = [vp, i32, C.c_char_p, C.POINTER(i64), C.POINTER(i32), C.POINTER(vp)]
    L.sqg_batch_run.restype = C.c_int
    L.sqg_batch_run.argtypes = [vp, vp]
    L.sqg_batch_wait.restype = C.c_int
    L.sqg_batch_wait.argtypes = [vp, vp, C.POINTER(CResult)]
    L.sqg_fetch_signal.restype = C.c_int
    L.sqg_fetch_signal.argtypes = [vp, vp, C.c_void_p]
    L.sqg_fetch_dwell.restype = C.c_int
    L.sqg_fetch_dwell.argtypes = [vp, vp, C.c_void_p]
    L.sqg_batch_free.restype = None
    L.sqg_batch_free.argtypes = [vp, vp]
    L.sqg_get_timing.restype = C.c_int
    L.sqg_get_timing.argtypes = [vp, C.POINTER(CTiming)]
    L.sqg_set_phase_timing.restype = C.c_int
    L.sqg_set_phase_timing.argtypes = [vp, C.c_int]
    L.sqg_submit.restype = C.c_int
    L.sqg_submit.argtypes = [vp, i32, C.c_char_p, C.POINTER(i64), C.POINTER(i32), C.POINTER(vp), C.POINTER(CResult)]
    L.sqg_worker_of.restype = i32
    L.sqg_worker_of.argtypes = [i32, i32, i32]
    L.sqg_probe_store_bandwidth.restype = C.c_int
    L.sqg_probe_store_bandwidth.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_float)]
    L.sqg_probe_lds_order.restype = C.c_int
    L.sqg_probe_lds_order.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_int)]
    L.sqg_batch_compress.restype = C.c_int
    L.sqg_batch_compress.argtypes = [vp, vp, C.POINTER(CSvb)]
    L.sqg_fetch_svb.restype = C.c_int
    L.sqg_fetch_svb.argtypes = [vp, vp, vp]
    L.sqg_genome_load.restype = C.c_int
    L.sqg_genome_load.argtypes = [vp, C.POINTER(CGenome)]
    L.sqg_genome_load_device.restype = C.c_int
    L.sqg_genome_load_device.argtypes = [vp, C.POINTER(CGenome)]
    L.sqg_genome_set_meth.restype = C.c_int
    L.sqg_genome_set_meth.argtypes = [vp, vp, vp]
    L.sqg_batch_sample.restype = C.c_int
    L.sqg_batch_sample.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(vp), C.POINTER(CSample)]
    L.sqg_fetch_reads.restype = C.c_int
    L.sqg_fetch_reads.argtypes = [vp, vp, vp]
    L.sqg_host_alloc.restype = vp
    L.sqg_host_alloc.argtypes = [C.c_size_t]
    L.sqg_host_free.restype = None
    L.sqg_host_free.argtypes = [vp]
    L.sqg_set_range_mode.restype = C.c_int
    L.sqg_set_range_mode.argtypes = [vp, C.c_int]
    L.sqg_skip_reads.restype = C.c_int
    L.sqg_skip_reads.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(i32)]
    L.sqg_batch_sample_range.restype = C.c_int
    L.sqg_batch_sample_range.argtypes = [vp, i32, C.POINTER(i32), i32, i32, C.POINTER(vp), C.POINTER(CSample)]
    L.sqg_batch_run_begin.restype = C.c_int
    L.sqg_batch_run_begin.argtypes = [vp, vp, C.POINTER(vp)]
    L.sqg_batch_run_end.restype = C.c_int
    L.sqg_batch_run_end.argtypes = [vp, vp, vp, vp]
    L.sqg_blow5_open.restype = C.c_int
    L.sqg_blow5_open.argtypes = [C.c_char_p, C.POINTER(CProfile), C.c_uint32, i32, C.POINTER(vp)]
    L.sqg_blow5_write.restype = C.c_int
    L.sqg_blow5_write.argtypes = [vp, i32, C.c_char_p, C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(i64), vp, C.POINTER(i64)]
    L.sqg_blow5_write_batch.restype = C.c_int
    L.sqg_blow5_write_batch.argtypes = [vp, vp, vp, C.c_char_p, C.POINTER(i64)]
    L.sqg_batch_blow5_records.restype = C.c_int
    L.sqg_batch_blow5_records.argtypes = [vp, vp, C.POINTER(CProfile), C.c_uint32, C.c_char_p, C.POINTER(i64), i64, C.c_uint64,
                                          C.POINTER(C.c_void_p), C.POINTER(i64), C.POINTER(C.POINTER(i64))]
    L.sqg_blow5_close.restype = C.c_int
    L.sqg_blow5_close.argtypes = [vp, C.POINTER(i64)]
    L.sqg_blow5_last_error.restype = C.c_char_p
    L.sqg_blow5_last_error.argtypes = [vp]
    L.sqg_set_stage_threads.restype = C.c_int
    L.sqg_set_stage_threads.argtypes = [vp, C.c_int]
    L.sqg_build_info.restype = C.c_char_p
    L.sqg_build_info.argtypes = []
    for names, table in _CONSUMER_EXPORTS:                  # each header's calls, when the library has them (the CPU backend has none)
        if all(hasattr(L, n) for n in names):
            for n in table:
                getattr(L, n).restype = C.c_int
                getattr(L, n).argtypes = [vp, vp] + [C.POINTER(t) for t in table[n]]
    if hasattr(L, "sqg_map_track"):
        L.sqg_map_track.restype = C.c_int
        L.sqg_map_track.argtypes = list(_MAP_TRACK_ARGS)
    _libs[path] = L
    return L


def _atoi(t: str) -> int:
    """C atoi: optional blanks and sign, then the leading digits (0 when there are none)"""
    import re
    m = re.match(r"\s*([+-]?\d+)", t)
    return int(m.group(1)) if m else 0


def _atof(t: str) -> float:
    """C atof: the longest leading decimal floating-point prefix (0.0 when there is none)"""
    import re
    m = re.match(r"\s*([+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?|inf(inity)?|nan))", t, re.I)
    return float(m.group(1)) if m else 0.0


def load_meth_freq(contigs, names, meth_freq_path: str):
    """load_meth_freq, src/ref.c:291-361: the --meth-freq table (tab separated: contig, 0-based position of a C, frequency in [0, 1])
    as one frequency byte per base of the concatenated contigs + a flag per contig; the reference's checks, as ValueError"""
    idx = {n: i for i, n in enumerate(names)}
    arrs = [np.zeros(len(c), np.uint8) for c in contigs]
    has = np.zeros(len(contigs), np.uint8)
    with open(meth_freq_path) as f:
        for line, ln in enumerate(f):
            if ln.startswith("#"):
                continue
            # the checks of load_meth_freq, src/ref.c:314-345 (the reference exits; here: ValueError naming the line)
            cols = ln.rstrip("\n").split("\t")
            if len(cols) < 3 or not all(cols[:3]):
                raise ValueError(f"{meth_freq_path}: malformed line {line} (need contig, position, frequency; src/ref.c:279-289)")
            name, pos, fr = cols[:3]
            if name not in idx:
                raise ValueError(f"There was no such chromosome in the reference. Check line {line} value {name} of the input methy-freq file.")
            i, p = idx[name], _atoi(pos)
            if p < 0:
                raise ValueError(f"Chromosome position cannot be negative. Check line {line} value {p} of the input methy-freq file.")
            if p >= len(contigs[i]):
                raise ValueError(f"Chromosome {name} position must be less than the length {len(contigs[i])}. Check line {line} value {p} "
                                 "of the input methy-freq file.")
            if contigs[i][p:p + 1] not in (b"C", b"c"):
                raise ValueError(f"The chromosome {name} position {p} in the reference was a {contigs[i][p:p + 1].decode()}. How can it be "
                                 f"methylated C? Check line {line} of the input methy-freq file.")
            fq = float(np.float32(_atof(fr)))
            if fq < 0 or fq > 1:
                raise ValueError(f"Methylation frequency must be between 0 to 1. Check line {line} value {fq:f} of the input methy-freq file.")
            has[i] = 1
            arrs[i][p] = int(np.floor(float(np.float32(fq) * np.float32(255)) + 0.5))     # (uint8_t)roundf(freq*255), float freq
    blob = np.concatenate(arrs) if arrs else np.zeros(1, np.uint8)
    return blob, has


class Blow5Writer:
    """The library's native BLOW5 writer (sqg_blow5_*): header, record framing and zlib on host threads; the signal field is
    the svb-zd encoding made on the device.  Pure host code: write() works without a GPU."""

    def __init__(self, path: str, profile: P.Profile, flags: int, threads: int = 0, lib_path: str | None = None, stored: bool = False, shards: int = 1,
                 huffman: bool = False):
        """stored: SQG_BLOW5_STORED -- the records in zlib streams of stored blocks, framed on the device by write_batch (include/sqg.h);
        huffman: SQG_BLOW5_HUFFMAN -- the records in zlib streams of two dynamic-Huffman blocks, coded on the device by write_batch and on
        the host threads by write (not with stored);
        shards > 1: SQG_BLOW5_SHARDS -- that many files (self.paths), each with a contiguous range of every batch's reads (stored or huffman)"""
        self.L = load_library(lib_path)
        self.h = C.c_void_p()
        cp = CProfile(*profile.as_tuple())
        self.paths = [path] if shards <= 1 else [(path[:-6] + f".{i}.blow5") if path.endswith(".blow5") else f"{path}.{i}" for i in range(shards)]
        rc = self.L.sqg_blow5_open(os.fsencode(path), C.byref(cp), (flags & (P.SQ_RNA | P.SQ_R10 | P.SQ_ONT)) | (BLOW5_STORED if stored else 0) | (BLOW5_HUFFMAN if huffman else 0)
                                   | ((shards & 0xff) << 24 if shards > 1 else 0), threads, C.byref(self.h))
        if rc != 0:
            raise SqgError(rc, "sqg_blow5_open", path)

    def _chk(self, rc, where):
        if rc != 0:
            raise SqgError(rc, where, self.L.sqg_blow5_last_error(self.h).decode())

    @staticmethod
    def _ids(read_ids):
        blob = b"".join(read_ids)
        off = np.zeros(len(read_ids) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in read_ids])
        return blob, off

    def write(self, read_ids, offset, median_before, sig_off, svb, svb_off):
        """read_ids: list of bytes; svb: uint8 array of the concatenated svb-zd encodings, svb_off their offsets"""
        blob, ioff = self._ids(read_ids)
        offset = np.ascontiguousarray(offset, np.float64); median_before = np.ascontiguousarray(median_before, np.float64)
        sig_off = np.ascontiguousarray(sig_off, np.int64); svb_off = np.ascontiguousarray(svb_off, np.int64)
        svb = np.ascontiguousarray(svb, np.uint8)
        dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int64)
        self._chk(self.L.sqg_blow5_write(self.h, len(read_ids), blob, ioff.ctypes.data_as(ip), offset.ctypes.data_as(dp),
                                         median_before.ctypes.data_as(dp), sig_off.ctypes.data_as(ip), svb.ctypes.data,
                                         svb_off.ctypes.data_as(ip)), "sqg_blow5_write")

    def write_batch(self, batch: "Batch", read_ids):
        blob, ioff = self._ids(read_ids)
        self._chk(self.L.sqg_blow5_write_batch(self.h, batch.gen.ctx, batch.handle, blob, ioff.ctypes.data_as(C.POINTER(C.c_int64))),
                  "sqg_blow5_write_batch")

    def close(self) -> int:
        n = C.c_int64()
        if self.h:
            rc = self.L.sqg_blow5_close(self.h, C.byref(n))
            self.h = None
            if rc != 0:
                raise SqgError(rc, "sqg_blow5_close")
        return n.value


class Batch:
    """A staged batch (one process_db() worth of reads)."""

    def __init__(self, gen, handle, n_reads):
        self.gen, self.handle, self.n_reads = gen, handle, n_reads
        self.res = None

    def _call(self, name, *args):
        """the library's `name` on this batch; SqgError with the context's text when it fails"""
        self.gen._chk(getattr(self.gen.L, name)(self.gen.ctx, self.handle, *args), name)

    def _plan(self, name, cfg):
        """(off [n_reads+1], total) of the plan call `name`: the first row of every read, their number"""
        off, total = np.zeros(self.n_reads + 1, np.int64), C.c_int64()
        self._call(name, C.byref(cfg), off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(total))
        return off, int(total.value)

    def _table(self, name, args, struct, names, shapes, want, tail=(), **head):
        """what sites / events / detect / align share: the Chunks of `head` and, for every output name, a zeroed tensor of its
        (shape, dtype) in `shapes` if it is wanted, else None; then the library's `name` with `args` and the C struct of their addresses"""
        import torch
        dev = torch.device("cuda", self.gen.device)
        ch = Chunks(**head, **{n: (torch.zeros(shapes[n][0], dtype=shapes[n][1], device=dev) if n in want else None) for n in names})
        out = _ptrs(struct, (getattr(ch, n) for n in names))
        torch.cuda.synchronize(dev)                         # (the zero fills and the caller's own work on its inputs, before another stream touches the blocks)
        self._call(name, *args, C.byref(out), *tail)
        return ch

    def run(self):
        self._call("sqg_batch_run")
        return self

    def run_begin(self) -> int:
        """Range sharding: first phase of the run; returns the DEVICE address of this range's per-stream sample counts
        (uint32 [num_workers][4^k], valid until the next run_begin)."""
        p = C.c_void_p()
        self._call("sqg_batch_run_begin", C.byref(p))
        return p.value

    def run_end(self, d_before: int | None = None, d_after: int | None = None):
        """second phase; d_before / d_after: device addresses of the counts summed over the earlier / later ranges"""
        self._call("sqg_batch_run_end", C.c_void_p(d_before), C.c_void_p(d_after))
        return self

    def wait(self):
        r = CResult()
        self._call("sqg_batch_wait", C.byref(r))
        self.res = r
        n = r.n_reads
        self.n_samples, self.n_events, self.n_bases = r.n_samples, r.n_events, r.n_bases
        self.sig_off = np.ctypeslib.as_array(r.sig_off, shape=(n + 1,)).copy()
        self.ev_off = np.ctypeslib.as_array(r.ev_off, shape=(n + 1,)).copy()
        self.offset = np.ctypeslib.as_array(r.offset, shape=(n,)).copy() if n else np.zeros(0)
        self.median_before = np.ctypeslib.as_array(r.median_before, shape=(n,)).copy() if n else np.zeros(0)
        return self

    def signal(self, out: np.ndarray | None = None) -> np.ndarray:
        """int16 samples of the batch; `out` may be (a view of) a pinned buffer from SignalGenerator.pinned()."""
        if out is None:
            out = np.empty(self.n_samples, np.int16)
        elif out.dtype != np.int16 or len(out) < self.n_samples:
            raise ValueError("destination too small for the batch's samples")
        self._call("sqg_fetch_signal", out.ctypes.data)
        return out[:self.n_samples]

    def dwell(self) -> np.ndarray:
        out = np.empty(self.n_events, np.int32)
        self._call("sqg_fetch_dwell", out.ctypes.data)
        return out

    def reads(self):
        """The sampled reads as gen_read returned them (list of bytes); only for batches made by sample()."""
        off = self.sampled["seq_off"]
        buf = np.empty(max(int(off[-1]), 1), np.uint8)
        self._call("sqg_fetch_reads", buf.ctypes.data)
        raw = buf.tobytes()
        return [raw[off[i]:off[i + 1]] for i in range(self.n_reads)]

    def compress(self, fetch=True, out: np.ndarray | None = None):
        """svb-zd encodings of the batch's signals (slow5lib's signal compression), made on the device.
        Returns (bytes as uint8 array, offsets[n_reads+1]); fetch=False leaves the bytes on the device."""
        r = CSvb()
        self._call("sqg_batch_compress", C.byref(r))
        off = np.ctypeslib.as_array(r.svb_off, shape=(self.n_reads + 1,)).copy()
        self._svb_bytes = int(r.n_bytes)
        if not fetch:
            return None, off
        return self.fetch_svb(out), off

    def fetch_svb(self, out: np.ndarray | None = None):
        """the encodings compress(fetch=False) left on the device (sqg_fetch_svb): a host that queues its next batch between the two
        calls has that batch's kernels running while these bytes cross PCIe"""
        n = getattr(self, "_svb_bytes", None)
        if n is None:
            raise ValueError("fetch_svb needs a compress() of this batch first")
        if out is not None and len(out) < n:
            raise ValueError("destination too small for the batch's encodings")
        out = np.empty(n, np.uint8) if out is None else out[:n]
        self._call("sqg_fetch_svb", out.ctypes.data)
        return out

    def blow5_records(self, profile, flags: int, read_ids, read_number0: int = 0, start_time0: int = 0):
        """the batch's BLOW5 records, framed on the device (sqg_batch_blow5_records) -> (bytes copy, offsets): in stored-block zlib streams,
        or -- BLOW5_HUFFMAN in flags -- in streams of two dynamic-Huffman blocks"""
        blob, ioff = Blow5Writer._ids(read_ids)
        cp = CProfile(*profile.as_tuple())
        recs, nb, ro = C.c_void_p(), C.c_int64(), C.POINTER(C.c_int64)()
        self._call("sqg_batch_blow5_records", C.byref(cp), flags, blob, ioff.ctypes.data_as(C.POINTER(C.c_int64)), read_number0, start_time0,
                   C.byref(recs), C.byref(nb), C.byref(ro))
        data = C.string_at(recs, nb.value) if nb.value else b""
        return data, np.array([ro[i] for i in range(len(read_ids) + 1)], np.int64)

    def signal_tensor(self):
        """zero-copy torch.int16 view of the batch's samples on the device (sqg_result_t.d_signal); valid as long as the batch's device
        results are (include/sqg.h: until two more batches have been run); the view keeps the batch alive"""
        import torch
        if self.res is None:
            self.wait()
        dev = torch.device("cuda", self.gen.device)
        if self.n_samples == 0:
            return torch.empty(0, dtype=torch.int16, device=dev)
        if not self.res.d_signal:
            raise SqgError(-4, "signal_tensor", "the batch's device results have been handed to a later batch")

        class _View:                                       # (the owner torch keeps: the batch stays alive with the tensor)
            def __init__(self, batch, ptr, n):
                self.batch = batch
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i2", "data": (ptr, False), "version": 2}
        return torch.as_tensor(_View(self, int(self.res.d_signal), int(self.n_samples)), device=dev)

    def _chunk_cfg(self, chunk_len, stride, max_label, dtype, norm):
        _need(self.gen.L, "sqg_batch_chunks", "sqg_chunks.h", "chunks")
        dt, nm = _enum("chunks", dtype=dtype, norm=norm)
        return CChunkCfg(int(chunk_len), int(chunk_len if stride is None else stride), int(max_label), dt, nm)

    def _trimmed(self, name, trim):
        """the library call `name`, or with trim its counterpart of include/sqg_segments.h (which cuts the inserts and takes SQG_PREFIX contexts)"""
        if not trim:
            return name
        _need(self.gen.L, "sqg_batch_segments", "sqg_segments.h", "segments")
        return name + "_trimmed"

    def segments(self):
        """(seg [n_reads, 5], shift [n_reads, 2]): int64 tensors on the batch's device -- every read's stall / adaptor / poly-A / insert
        bounds in stored samples and the range of the RNA adaptor's level shift (sqg_batch_segments, include/sqg_segments.h)"""
        import torch
        self._trimmed("", True)
        shapes = dict(seg=((self.n_reads, 5), torch.int64), shift=((self.n_reads, 2), torch.int64))
        sg = self._table("sqg_batch_segments", (), CSegments, tuple(shapes), shapes, shapes)
        return sg.seg, sg.shift

    def chunk_plan(self, chunk_len: int, stride: int | None = None, trim: bool = False):
        """(chunk_off [n_reads+1], n_chunks): the first chunk of every read, from the batch's sig_off (sqg_chunk_plan; host only).
        trim=True: of every read's insert (sqg_chunk_plan_trimmed, include/sqg_segments.h; device work)"""
        cfg = self._chunk_cfg(chunk_len, stride, 0, CHUNK_F16, CHUNK_MEDMAD)
        return self._plan(self._trimmed("sqg_chunk_plan", trim), cfg)

    def _chunk_job(self, chunk_len, stride, max_label, dtype, norm, trim=False):
        """what chunks() and chunk_targets() share: (cfg, chunk_off, n_chunks, device, new, call) -- new(shape, dtype): an output tensor;
        call(name, out, *tensors): the C struct `out` filled with the tensors' addresses, then the library's `name` on this batch"""
        import torch
        cfg = self._chunk_cfg(chunk_len, stride, max_label, dtype, norm)
        off, nc = self.chunk_plan(chunk_len, cfg.stride, trim)
        dev = torch.device("cuda", self.gen.device)
        new = lambda shape, dt: (torch.zeros if nc == 0 else torch.empty)(shape, dtype=dt, device=dev)   # noqa: E731
        def call(name, out, *tensors):
            out = _ptrs(out, tensors)
            torch.cuda.synchronize(dev)                     # (the allocator's pending work on these blocks, if any, before another stream writes them)
            self._call(self._trimmed(name, trim), C.byref(cfg), C.byref(out))
        return cfg, off, nc, dev, new, call

    def chunks(self, chunk_len: int, stride: int | None = None, max_label: int = 0, dtype="f16", norm="medmad",
               signal: bool = True, labels: bool = True, trim: bool = False) -> Chunks:
        """Fixed-length, per-read normalised windows of the batch's signal and their base labels, made on the device
        (sqg_batch_chunks): torch tensors signal [n_chunks, L] (float16 / float32), labels [n_chunks, W] (uint8, 0 = padding),
        label_len, chunk_read, chunk_start [n_chunks], med2, mad4 [n_reads].  signal=False / labels=False leave those passes out
        (the tensors are then None).  trim=True: chunks of every read's insert, the way into SQG_PREFIX contexts
        (sqg_batch_chunks_trimmed, include/sqg_segments.h)."""
        import torch
        cfg, off, nc, dev, new, call = self._chunk_job(chunk_len, stride, max_label, dtype, norm, trim)
        ch = Chunks(n_chunks=nc, chunk_off=off,
                    signal=new((nc, cfg.chunk_len), torch.float32 if cfg.dtype == CHUNK_F32 else torch.float16) if signal else None,
                    labels=new((nc, cfg.max_label), torch.uint8) if labels else None,
                    label_len=new((nc,), torch.int32) if labels else None,
                    chunk_read=new((nc,), torch.int32), chunk_start=new((nc,), torch.int64),
                    med2=torch.zeros(self.n_reads, dtype=torch.int32, device=dev), mad4=torch.zeros(self.n_reads, dtype=torch.int32, device=dev))
        if self.n_reads:                                    # (also for a plan without chunks: med2 / mad4 are written for every read)
            call("sqg_batch_chunks", CChunkOut, ch.signal, ch.labels, ch.label_len, ch.chunk_read, ch.chunk_start, ch.med2, ch.mad4)
        return ch

    def chunk_targets(self, chunk_len: int, stride: int | None = None, dtype="f16", norm="medmad", clean: bool = True,
                      clean_raw: bool = False, moves: bool = True, kmer: bool = False, chunks: Chunks | None = None,
                      trim: bool = False) -> Chunks:
        """Per-sample targets for the chunks Batch.chunks() cuts with the same chunk_len / stride (sqg_batch_chunk_targets,
        include/sqg_targets.h): torch tensors [n_chunks, L] on the batch's device -- clean (float16 / float32: the noise-free signal on
        the noisy read's scale), clean_raw (int16: what --ideal-amp writes), moves (uint8: 1 where an event starts), kmer (uint32 bit
        patterns in an int32 tensor: the pore-table row).  Those not asked for are None.  chunks=: a Chunks of this batch, whose med2 /
        mad4 are passed in instead of being computed again.  trim=True: for the chunks of chunks(..., trim=True)
        (sqg_batch_chunk_targets_trimmed, include/sqg_segments.h)."""
        import torch
        _need(self.gen.L, "sqg_batch_chunk_targets", "sqg_targets.h", "chunk_targets")
        cfg, off, nc, dev, new, call = self._chunk_job(chunk_len, stride, 0, dtype, norm, trim)
        row = lambda want, dt: new((nc, cfg.chunk_len), dt) if want else None           # noqa: E731
        tg = Chunks(n_chunks=nc, chunk_off=off, clean=row(clean, torch.float32 if cfg.dtype == CHUNK_F32 else torch.float16),
                    clean_raw=row(clean_raw, torch.int16), moves=row(moves, torch.uint8), kmer=row(kmer, torch.int32))
        if nc == 0:
            return tg
        st = (None, None)
        if chunks is not None:
            st = (getattr(chunks, "med2", None), getattr(chunks, "mad4", None))
            for t in st:                                    # (a Chunks of another batch or device would silently put clean on a wrong scale)
                if t is None or t.dtype != torch.int32 or t.device != dev or t.numel() != self.n_reads or not t.is_contiguous():
                    raise SqgError(-1, "chunk_targets", f"chunks= must carry this batch's med2 / mad4: int32 [{self.n_reads}] on {dev}")
        call("sqg_batch_chunk_targets", CChunkTargets, tg.clean, tg.clean_raw, tg.moves, tg.kmer, *st)
        return tg

    def _site_cfg(self, win_len, before, focus, ctx_len, ctx_before, dtype, norm):
        _need(self.gen.L, "sqg_batch_sites", "sqg_sites.h", "sites")
        dt, nm = _enum("sites", dtype=dtype, norm=norm)
        L, B = int(win_len), int(ctx_len)
        return CSiteCfg(L, int(L // 2 if before is None else before), int(self.gen.kmer_size // 2 if focus is None else focus), B,
                        int(B // 2 if ctx_before is None else ctx_before), dt, nm)

    def site_plan(self, win_len: int, before: int | None = None, focus: int | None = None):
        """(site_off [n_reads+1], n_sites): the first CpG site of every read for windows of win_len samples, `before` of them in front of
        the anchor event (default win_len / 2), the site's base at position `focus` of that event's k-mer (default k / 2)
        (sqg_site_plan, include/sqg_sites.h; device work and a copy-back of the per-read counts)"""
        return self._plan("sqg_site_plan", self._site_cfg(win_len, before, focus, 0, 0, CHUNK_F16, CHUNK_MEDMAD))

    def sites(self, win_len: int, before: int | None = None, focus: int | None = None, ctx_len: int = 0, ctx_before: int | None = None,
              dtype="f16", norm="medmad", outputs=None) -> Chunks:
        """One normalised window of signal around every CpG site of the batch with the site's methylation label, made on the device
        (sqg_batch_sites, include/sqg_sites.h): torch tensors signal [n_sites, L] (float16 / float32), label (uint8: 1 where the read
        carries 'M'), site_read, site_pos (int32), win_start (int64) [n_sites], context [n_sites, B] (uint8 label codes around the
        site), ctx_start [n_sites, B + 1] (int32: where each context base's samples start in the window), med2, mad4 [n_reads].
        before / focus / ctx_before default to win_len / 2, k / 2, ctx_len / 2.  outputs: the names wanted (default all); the others are None."""
        import torch
        cfg = self._site_cfg(win_len, before, focus, ctx_len, ctx_before, dtype, norm)
        want = _want(outputs, SITE_OUTPUTS, "sites")
        off, ns = self._plan("sqg_site_plan", cfg)          # (validates all of cfg: the shapes below are sane)
        L, B = cfg.win_len, cfg.ctx_len
        shapes = dict(signal=((ns, L), torch.float32 if cfg.dtype == CHUNK_F32 else torch.float16), label=((ns,), torch.uint8),
                      site_read=((ns,), torch.int32), site_pos=((ns,), torch.int32), win_start=((ns,), torch.int64),
                      context=((ns, B), torch.uint8), ctx_start=((ns, B + 1), torch.int32),
                      med2=((self.n_reads,), torch.int32), mad4=((self.n_reads,), torch.int32))
        return self._table("sqg_batch_sites", (C.byref(cfg),), CSiteOut, SITE_OUTPUTS, shapes, want, n_sites=ns, site_off=off)

    def events(self, norm="pa", trim: bool = False, outputs=None) -> Chunks:
        """The per-event signal table of the batch, made on the device (sqg_batch_events, include/sqg_events.h): one row per event in
        the order of dwell(), read r's rows being [ev_off[r], ev_off[r+1]).  torch tensors [n_events]: ev_read (int32), ev_start (int64:
        first stored sample within the read), ev_len (int32), sum, sumsq (int64), vmin, vmax (int16), kmer (uint32 bit patterns in an
        int32 tensor: the pore-table row), level_raw (int16), seg (uint8: 0 stall, 1 adaptor, 2 poly-A, 3 insert), mean, sd (float32,
        normalised by norm: "pa" or "medmad"); med2, mad4 [n_reads] (int32), over the whole read or with trim over its insert.
        outputs: the names wanted (default all); the others are None."""
        import torch
        _need(self.gen.L, "sqg_batch_events", "sqg_events.h", "events")
        nm, = _enum("events", norm=norm)
        want = _want(outputs, EVENT_OUTPUTS, "events")
        cfg = CEventCfg(nm, int(trim))
        ne = self._n_events()
        dts = dict(ev_read=torch.int32, ev_start=torch.int64, ev_len=torch.int32, sum=torch.int64, sumsq=torch.int64, vmin=torch.int16, vmax=torch.int16,
                   kmer=torch.int32, level_raw=torch.int16, seg=torch.uint8, mean=torch.float32, sd=torch.float32, med2=torch.int32, mad4=torch.int32)
        shapes = {n: (self.n_reads if n in ("med2", "mad4") else ne, dt) for n, dt in dts.items()}
        return self._table("sqg_batch_events", (C.byref(cfg),), CEventOut, EVENT_OUTPUTS, shapes, want, n_events=ne)

    def _detect_cfg(self, cfg, norm, trim):
        _need(self.gen.L, "sqg_batch_detect", "sqg_detect.h", "detect")
        nm, = _enum("detect", norm=norm)
        five = DETECT_PRESETS.get(cfg, cfg) if isinstance(cfg, str) else cfg
        if isinstance(five, str) or len(five) != 5:
            raise SqgError(-1, "detect", f"cfg must be one of {sorted(DETECT_PRESETS)} or (w_short, w_long, thr_short, thr_long, peak_height), not {cfg!r}")
        return CDetectCfg(int(five[0]), int(five[1]), float(five[2]), float(five[3]), float(five[4]), nm, int(trim))

    def detect_plan(self, cfg="dna"):
        """(det_off [n_reads+1], n_rows): the first row of every read in the table Batch.detect() makes with the same cfg
        (sqg_detect_plan, include/sqg_detect.h; device work and a copy-back of the per-read counts)"""
        return self._plan("sqg_detect_plan", self._detect_cfg(cfg, "pa", False))

    def detect(self, cfg="dna", norm="pa", trim: bool = False, outputs=None) -> Chunks:
        """The table a raw-signal tool's event detector finds in the batch's stored samples, made on the device (sqg_batch_detect,
        include/sqg_detect.h): the two-window t-statistic detector of scrappie / f5c with exact integer window sums.  cfg: "dna", "rna"
        or (w_short, w_long, thr_short, thr_long, peak_height).  torch tensors [n_rows]: dt_read (int32), dt_start (int64: first stored
        sample within the read), dt_len (int32), sum, sumsq (int64), vmin, vmax (int16), mean, sd (float32, normalised by norm: "pa"
        or "medmad"), true_ev (int64: the row of Batch.events() under the row's first sample); med2, mad4 [n_reads] (int32), over the
        whole read or with trim over its insert; det_off (numpy, [n_reads+1]) and n_rows from the plan.
        outputs: the names wanted (default all); the others are None."""
        import torch
        c = self._detect_cfg(cfg, norm, trim)
        want = _want(outputs, DETECT_OUTPUTS, "detect")
        off, nr = self._plan("sqg_detect_plan", c)          # (validates all of cfg, and that the batch has been run)
        dts = dict(dt_read=torch.int32, dt_start=torch.int64, dt_len=torch.int32, sum=torch.int64, sumsq=torch.int64, vmin=torch.int16, vmax=torch.int16,
                   mean=torch.float32, sd=torch.float32, true_ev=torch.int64, med2=torch.int32, mad4=torch.int32)
        shapes = {n: (self.n_reads if n in ("med2", "mad4") else nr, dt) for n, dt in dts.items()}
        return self._table("sqg_batch_detect", (C.byref(c),), CDetectOut, DETECT_OUTPUTS, shapes, want, n_rows=nr, det_off=off)

    def align(self, row_off, sum, len, cfg=None, outputs=None, scale=None) -> Chunks:       # noqa: A002  (the header's names)
        """The rows [row_off[r], row_off[r+1]) of sum / len -- Batch.detect()'s det_off, sum and dt_len, or any other segmentation of the
        reads -- aligned to the true events of read r by a banded dynamic programme in exact integers, on the device (sqg_batch_align,
        include/sqg_align.h).  row_off: [n_reads+1] integers on the host; sum (int64) and len (int32): torch tensors of row_off[-1]
        elements on the context's device.  cfg: (stay_pen, skip_pen, cost_cap), default SQG_ALIGN_DEFAULT.  torch tensors al_ev
        [n_rows] (int64: the row of Batch.events() a row is aligned to, -1: none), al_cost [n_reads] (int64: the cost of the read's best
        path, -1: none), al_edge [n_reads] (int32: rows on the moving band's rim).  outputs: the names wanted (default all); the others
        are None.  scale=(gain, shift): int32 tensors [n_reads] on the context's device, a row's level taken as (gain * q >> 16) + shift
        (gain in Q16, shift in 1/256 code: Batch.scale()'s estimate, sqg_batch_align_scaled, include/sqg_scale.h); None: the rows as they stand."""
        import torch
        _need(self.gen.L, "sqg_batch_align", "sqg_align.h", "align")
        if scale is not None:
            _need(self.gen.L, "sqg_batch_align_scaled", "sqg_scale.h", "align")
        three = ALIGN_DEFAULT if cfg is None else cfg
        if isinstance(three, str) or _len(three) != 3:
            raise SqgError(-1, "align", f"cfg must be (stay_pen, skip_pen, cost_cap), not {cfg!r}")
        c = CAlignCfg(*(int(v) for v in three))
        want = _want(outputs, ALIGN_OUTPUTS, "align")
        off, nr, cin, keep = self._rows("align", row_off, CAlignIn, (sum, len))
        dev = torch.device("cuda", self.gen.device)
        shapes = dict(al_ev=(nr, torch.int64), al_cost=(self.n_reads, torch.int64), al_edge=(self.n_reads, torch.int32))
        args = (C.byref(c), off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cin))
        if scale is None:
            return self._table("sqg_batch_align", args, CAlignOut, ALIGN_OUTPUTS, shapes, want, n_rows=nr, row_off=off)
        if isinstance(scale, torch.Tensor) or _len(scale) != 2:
            raise SqgError(-1, "align", "scale must be (gain, shift)")
        for name, t in zip(("gain", "shift"), scale):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == dev and t.is_contiguous() and t.numel() == self.n_reads):
                raise SqgError(-1, "align", f"scale: {name} must be a contiguous {torch.int32} tensor of {self.n_reads} elements on {dev}")
        csc = CAlignScale(*(t.data_ptr() if t.numel() else keep.data_ptr() for t in scale))
        return self._table("sqg_batch_align_scaled", args + (C.byref(csc),), CAlignOut, ALIGN_OUTPUTS, shapes, want, n_rows=nr, row_off=off)

    def scale(self, row_off, sum, len, ev=None, mode=None, outputs=None) -> Chunks:       # noqa: A002  (the header's names)
        """The per-read shift and scale a tool would estimate from the rows [row_off[r], row_off[r+1]) of sum / len, on the device
        (sqg_batch_scale, include/sqg_scale.h).  mode "moments" (the default without ev): the rows' mean and variance against those of ALL
        the read's true events.  mode "fit" (the default with ev): least squares of the event's level on the row's over the rows that ev
        -- Batch.align()'s al_ev, the detector's true_ev, or the caller's own -- assigns to an event of their own read; the others are
        dropped.  row_off: [n_reads+1] integers on the host; sum, ev (int64) and len (int32): torch tensors of row_off[-1] elements on the
        context's device.  torch tensors [n_reads]: n, nx, sy, syy, sx, sxx, sxy (int64: the exact sums in 1/16 code), gain (int32, Q16),
        shift (int32, 1/256 code) -- what Batch.align(scale=(gain, shift)) takes; the truth of a simulated read is (65536, 0) --,
        rd_dropped (int32).  outputs: the names wanted (default all); the others are None."""
        import torch
        _need(self.gen.L, "sqg_batch_scale", "sqg_scale.h", "scale")
        md, = _enum("scale", mode=("moments" if ev is None else "fit") if mode is None else mode)
        want = _want(outputs, SCALE_OUTPUTS, "scale")
        off, nr, cin, keep = self._rows("scale", row_off, CScaleIn, (sum, len, ev), ("ev",))
        c = CScaleCfg(md)
        shapes = {n: (self.n_reads, torch.int32 if n in ("gain", "shift", "rd_dropped") else torch.int64) for n in SCALE_OUTPUTS}
        return self._table("sqg_batch_scale", (C.byref(c), off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cin)), CScaleOut, SCALE_OUTPUTS, shapes, want,
                           n_rows=nr, row_off=off)

    def _rows(self, who, row_off, struct, cols, optional=()):
        """the caller's rows of align() / scale() / collapse() / pileup_rows(): row_off, and cols, a tensor for every field of the call's C
        `struct` in its order (int64, `len` int32); one named in `optional` may be None (the library says what needs it).  Returns (row_off
        as int64, n_rows, the struct of the columns' addresses, what keeps them valid until the library call has returned)"""
        import torch
        off = np.ascontiguousarray(row_off, np.int64)
        if off.shape != (self.n_reads + 1,):
            raise SqgError(-1, who, f"row_off must have {self.n_reads + 1} elements")
        nr = max(int(off[-1]), 0)
        dev = torch.device("cuda", self.gen.device)
        for (name, _), t in zip(struct._fields_, cols):
            dt = torch.int32 if name == "len" else torch.int64
            if t is None and name in optional:
                continue
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.device == dev and t.is_contiguous() and t.numel() >= nr):
                raise SqgError(-1, who, f"{name} must be a contiguous {dt} tensor of at least {nr} elements on {dev}")
        keep = torch.zeros(1, dtype=torch.int64, device=dev)  # (a valid address for an empty table: NULL is an error, and nothing is read)
        return off, nr, struct(*(None if t is None else t.data_ptr() if t.numel() else keep.data_ptr() for t in cols)), keep

    def _n_events(self):
        """a table's row count; a batch not yet waited for is waited for here (one not run: 0, and the library's SQG_ESEQUENCE behind)"""
        if self.res is None and self.handle:
            r = CResult()
            return int(r.n_events) if self.gen.L.sqg_batch_wait(self.gen.ctx, self.handle, C.byref(r)) == 0 else 0
        return int(self.n_events)

    def collapse(self, row_off, ev, sum, sumsq, len, norm="pa", trim: bool = False, outputs=None) -> Chunks:       # noqa: A002  (the header's names)
        """The observed event table: the rows [row_off[r], row_off[r+1]) of sum / sumsq / len -- Batch.detect()'s det_off, sum, sumsq and
        dt_len, or any other -- summed per row of Batch.events() they are assigned to by ev -- Batch.align()'s al_ev, the detector's
        true_ev, or the caller's own -- on the device (sqg_batch_collapse, include/sqg_collapse.h).  A row whose ev is not an event of its
        own read is dropped.  row_off: [n_reads+1] integers on the host; ev, sum, sumsq (int64) and len (int32): torch tensors of
        row_off[-1] elements on the context's device; sumsq may be None when neither ob_sumsq nor sd is wanted.  torch tensors [n_events]:
        ob_rows (uint32 bit patterns in an int32 tensor), ob_len, ob_sum, ob_sumsq (int64), mean, sd (float32: the event table's formulas
        on the sums, normalised by norm, 0 for an event without a sample); rd_dropped [n_reads] (int32).  outputs: the names wanted
        (default all); the others are None."""
        import torch
        _need(self.gen.L, "sqg_batch_collapse", "sqg_collapse.h", "collapse")
        nm, = _enum("collapse", norm=norm)
        want = _want(outputs, COLLAPSE_OUTPUTS, "collapse")
        off, nr, cin, keep = self._rows("collapse", row_off, CCollapseIn, (ev, sum, sumsq, len), ("sumsq",))
        c = CCollapseCfg(nm, int(trim))
        ne = self._n_events()
        dts = dict(ob_rows=torch.int32, ob_len=torch.int64, ob_sum=torch.int64, ob_sumsq=torch.int64, mean=torch.float32, sd=torch.float32, rd_dropped=torch.int32)
        shapes = {n: (self.n_reads if n == "rd_dropped" else ne, dt) for n, dt in dts.items()}
        return self._table("sqg_batch_collapse", (C.byref(c), off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cin)), CCollapseOut, COLLAPSE_OUTPUTS, shapes, want,
                           n_rows=nr, row_off=off, n_events=ne)

    def call_plan(self):
        """(site_off [n_reads+1], n_sites): the first CpG site of every read as Batch.call() numbers them (sqg_call_plan, include/sqg_call.h;
        device work and a copy-back of the per-read counts)"""
        _need(self.gen.L, "sqg_call_plan", "sqg_call.h", "call")
        off, total = np.zeros(self.n_reads + 1, np.int64), C.c_int64()
        self._call("sqg_call_plan", off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(total))
        return off, int(total.value)

    def call(self, sum, len, model=None, scale=None, origin=None, freq=None, outputs=None, **cfg) -> Chunks:       # noqa: A002  (the header's names)
        """Per-read CpG methylation calls of the batch, scored on the device from one row of (sum, len) per row of Batch.events()
        (sqg_batch_call, include/sqg_call.h): the events whose k-mer holds a CpG's C are scored under the pore model's rows with C and with
        M there, in exact integers.  sum (int64) and len (int32: Batch.events()'s ev_len; or int64: Batch.collapse()'s ob_len, an event
        with len < 1 is unobserved): torch tensors of n_events elements on the context's device.  model=(w, c): int32 tensors [5^k]
        (default SignalGenerator.call_model()).  scale=(gain, shift) as in Batch.align().  origin=(key0, step) as in Batch.pileup()
        (default: the sampler's).  freq: a CallFreq of SignalGenerator.new_call_freq(), added to.  cfg by keyword: neigh ("same" | "read"),
        term_cap, llr_min, min_obs (default SQG_CALL_DEFAULT).  torch tensors [n_sites]: site_read, site_pos (int32), label (uint8),
        site_key (int64), n_obs, nll_c, nll_m, llr (int32, 1/256 nat; llr > 0 speaks for M), call (uint8: 0 none, 1 unmethylated,
        2 methylated); site_off (numpy, [n_reads+1]) and n_sites from the plan; stat = (sites, outside, called, agree).
        outputs: the names wanted (default all, site_key only where there is an origin); the others are None."""
        import torch
        _need(self.gen.L, "sqg_batch_call", "sqg_call.h", "call")
        if set(cfg) - {"neigh", "term_cap", "llr_min", "min_obs"}:
            raise SqgError(-1, "call", f"unknown cfg {sorted(set(cfg) - {'neigh', 'term_cap', 'llr_min', 'min_obs'})}")
        ng, = _enum("call", neigh=cfg.get("neigh", CALL_DEFAULT[0]))
        c = CCallCfg(ng, *(int(cfg.get(n, d)) for n, d in zip(("term_cap", "llr_min", "min_obs"), CALL_DEFAULT[1:])))
        dev = torch.device("cuda", self.gen.device)
        ne = self._n_events()
        keep = torch.zeros(1, dtype=torch.int64, device=dev)    # (a valid address for an empty table: NULL is an error, and nothing is read)

        def addr(name, t, dts, n):
            if not (isinstance(t, torch.Tensor) and t.dtype in dts and t.device == dev and t.is_contiguous() and t.numel() >= n):
                raise SqgError(-1, "call", f"{name} must be a contiguous {' or '.join(str(d) for d in dts)} tensor of at least {n} elements on {dev}")
            return t.data_ptr() if t.numel() else keep.data_ptr()
        a_sum, a_len = addr("sum", sum, (torch.int64,), ne), addr("len", len, (torch.int32, torch.int64), ne)
        cin = CCallIn(a_sum, a_len if len.dtype == torch.int64 else None, a_len if len.dtype == torch.int32 else None)
        if model is None:
            model = self.gen.call_model()
        if isinstance(model, torch.Tensor) or _len(model) != 2:
            raise SqgError(-1, "call", "model must be (w, c)")
        rows = 5 ** self.gen.kmer_size
        cmod = CCallModel(*(addr(f"model: {n}", t, (torch.int32,), rows) for n, t in zip(("w", "c"), model)))
        csc = None
        if scale is not None:
            if isinstance(scale, torch.Tensor) or _len(scale) != 2:
                raise SqgError(-1, "call", "scale must be (gain, shift)")
            csc = CAlignScale(*(addr(f"scale: {n}", t, (torch.int32,), self.n_reads) for n, t in zip(("gain", "shift"), scale)))
        org, held = self._origin("call", origin)
        keyed = origin is not None or hasattr(self, "sampled")
        want = _want(outputs, CALL_OUTPUTS, "call") if outputs is not None or keyed else set(CALL_OUTPUTS) - {"site_key"}
        cfq = None
        if freq is not None:
            cfq = CCallFreq(int(freq.lo), int(freq.hi), *(t.data_ptr() if t is not None and t.numel() else None for t in (getattr(freq, n) for n in CALL_FREQ)))
        off, ns = self.call_plan()
        st = CCallStat()
        dts = dict(site_read=torch.int32, site_pos=torch.int32, label=torch.uint8, site_key=torch.int64, n_obs=torch.int32, nll_c=torch.int32,
                   nll_m=torch.int32, llr=torch.int32, call=torch.uint8)
        ref = lambda s: C.byref(s) if s is not None else None     # noqa: E731
        ch = self._table("sqg_batch_call", (C.byref(c), C.byref(cin), C.byref(cmod), ref(csc), ref(org)), CCallOut, CALL_OUTPUTS,
                         {n: (ns, dt) for n, dt in dts.items()}, want, tail=(ref(cfq), C.byref(st)), n_sites=ns, site_off=off)
        ch.stat = (int(st.sites), int(st.outside), int(st.called), int(st.agree))
        return ch

    def map_shift(self):
        """(gain, shift): the scale that puts this batch's rows in stored ADC codes on the scale of SignalGenerator.map_levels() -- gain 65536
        and shift rint(256 * offset[r]) from the offsets the host already has --, int32 tensors [n_reads] on the context's device: what
        Batch.map(scale=...) takes (include/sqg_map.h; a binding recommendation, not part of the kernel's rule)"""
        import torch
        _need(self.gen.L, "sqg_batch_map", "sqg_map.h", "map")
        if self.res is None:
            self.wait()
        dev = torch.device("cuda", self.gen.device)
        shift = np.clip(np.rint(256.0 * np.asarray(self.offset, np.float64)), -(1 << 26), 1 << 26).astype(np.int32)
        return torch.full((self.n_reads,), 65536, dtype=torch.int32, device=dev), torch.from_numpy(shift).to(dev)

    def map(self, row_off, sum, len, track, cfg=None, scale=None, outputs=None) -> Chunks:       # noqa: A002  (the header's names)
        """The first rows of every read -- rows [row_off[r] + row_first, ...) of sum / len, at most row_count of them -- mapped against the
        level track of a genome window by subsequence DTW in exact integers, on the device (sqg_batch_map, include/sqg_map.h).  row_off, sum
        and len as in Batch.align().  track: a MapTrack (SignalGenerator.new_map_track(), or synthetic tensors).  cfg: (stay_pen, skip_pen,
        cost_cap, row_first, row_count, strands), default SQG_MAP_DEFAULT.  scale=(gain, shift) as in Batch.align(); Batch.map_shift() is the
        one for rows in stored codes against map_levels().  torch tensors [n_reads]: map_cost (int32), map_step (int8: +1 / -1, 0 none),
        map_key0, map_key1 (int64: the forward coordinate of the k-mer under row 0 / the last row), map_cost_other (int32).  outputs: the
        names wanted (default all); the others are None."""
        import torch
        _need(self.gen.L, "sqg_batch_map", "sqg_map.h", "map")
        six = MAP_DEFAULT if cfg is None else cfg
        if isinstance(six, str) or _len(six) != 6:
            raise SqgError(-1, "map", f"cfg must be ({', '.join(MAP_CFG)}), not {cfg!r}")
        c = CMapCfg(*(int(v) for v in six[:5]), int(six[5]) & 0xffffffff)
        want = _want(outputs, MAP_OUTPUTS, "map")
        off, nr, cin, keep = self._rows("map", row_off, CAlignIn, (sum, len))
        dev = torch.device("cuda", self.gen.device)
        if not isinstance(track, MapTrack):
            raise SqgError(-1, "map", "track must be a MapTrack")
        w = max(track.hi - track.lo, 0)
        for name in ("fwd", "rev"):
            t = getattr(track, name)
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == dev and t.is_contiguous() and t.numel() >= w):
                raise SqgError(-1, "map", f"track: {name} must be a contiguous {torch.int32} tensor of at least {w} elements on {dev}")
        ctr = CMapTrack(track.lo, track.hi, *(None if t is None else t.data_ptr() if t.numel() else keep.data_ptr() for t in (track.fwd, track.rev)))
        csc = None
        if scale is not None:
            if isinstance(scale, torch.Tensor) or _len(scale) != 2:
                raise SqgError(-1, "map", "scale must be (gain, shift)")
            for name, t in zip(("gain", "shift"), scale):
                if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == dev and t.is_contiguous() and t.numel() == self.n_reads):
                    raise SqgError(-1, "map", f"scale: {name} must be a contiguous {torch.int32} tensor of {self.n_reads} elements on {dev}")
            csc = CAlignScale(*(t.data_ptr() if t.numel() else keep.data_ptr() for t in scale))
        dts = dict(map_cost=torch.int32, map_step=torch.int8, map_key0=torch.int64, map_key1=torch.int64, map_cost_other=torch.int32)
        args = (C.byref(c), off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cin), C.byref(csc) if csc is not None else None, C.byref(ctr))
        return self._table("sqg_batch_map", args, CMapOut, MAP_OUTPUTS, {n: (self.n_reads, dt) for n, dt in dts.items()}, want, row_off=off)

    def _origin(self, who, origin):
        """the C origin of pileup() / pileup_rows() (None: the sampler's) and the arrays it points into"""
        if origin is None:
            return None, None
        key0, step = np.ascontiguousarray(origin[0], np.int64), np.ascontiguousarray(origin[1], np.int8)
        if key0.shape != (self.n_reads,) or step.shape != (self.n_reads,):
            raise SqgError(-1, who, f"origin=(key0, step) must be two arrays of {self.n_reads} elements")
        return COrigin(key0.ctypes.data_as(C.POINTER(C.c_int64)), step.ctypes.data_as(C.POINTER(C.c_int8))), (key0, step)

    def pileup_rows(self, p: Pileup, row_off, ev, sum, sumsq, len, origin=None):       # noqa: A002
        """Adds the OBSERVED events of the rows -- those of collapse(), taken the same way -- to the pileup `p` of
        SignalGenerator.new_pileup() under the rules of Batch.pileup() (sqg_batch_pileup_rows, include/sqg_collapse.h): one count per event
        that has a row, its dwell the rows' samples, mean and sd those of collapse() under p's norm and trim.  Returns (counted, outside,
        unseen, dropped): unseen are the events that would count and have no row, dropped the rows that are assigned to no event of their
        read.  origin as in pileup()."""
        import torch
        _need(self.gen.L, "sqg_batch_pileup_rows", "sqg_collapse.h", "pileup_rows")
        off, _, cin, keep = self._rows("pileup_rows", row_off, CCollapseIn, (ev, sum, sumsq, len), ("sumsq",))
        org, held = self._origin("pileup_rows", origin)
        out = _ptrs(CPileupOut, (getattr(p, n) for n in PILEUP_OUTPUTS))
        st = CPileupRowsStat()
        torch.cuda.synchronize(torch.device("cuda", self.gen.device))     # (the zero fills or the caller's own work on the sums and the rows, before another stream touches them)
        self._call("sqg_batch_pileup_rows", C.byref(p.cfg), C.byref(org) if org is not None else None, off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cin),
                   C.byref(out), C.byref(st))
        return int(st.counted), int(st.outside), int(st.unseen), int(st.dropped)

    def pileup(self, p: Pileup, origin=None):
        """Adds the batch's events to the pileup `p` of SignalGenerator.new_pileup() (sqg_batch_pileup, include/sqg_pileup.h) and returns
        (counted, outside).  origin=(key0, step): numpy arrays [n_reads] (int64, int8) in place of the sampler's origin -- for staged
        batches, or another coordinate system"""
        import torch
        _need(self.gen.L, "sqg_batch_pileup", "sqg_pileup.h", "pileup")
        org, held = self._origin("pileup", origin)
        out = _ptrs(CPileupOut, (getattr(p, n) for n in PILEUP_OUTPUTS))
        st = CPileupStat()
        torch.cuda.synchronize(torch.device("cuda", self.gen.device))     # (the zero fills or the caller's own work on the sums, before another stream adds to them)
        self._call("sqg_batch_pileup", C.byref(p.cfg), C.byref(org) if org is not None else None, C.byref(out), C.byref(st))
        return int(st.counted), int(st.outside)

    def free(self):
        if self.handle:
            self.gen.L.sqg_batch_free(self.gen.ctx, self.handle)
            self.handle = None

    def __del__(self):
        try:
            if self.gen.ctx:
                self.free()
        except Exception:
            pass


class SignalGenerator:
    """One simulation context: the reference's core_t for (profile, flags, model, seed, -t)."""

    def __init__(self, profile: P.Profile, flags: int, kmer_size: int, level_mean, level_stdv, seed: int,
                 num_workers: int = 1, amp_noise: float = 1.0, device: int = 0, mode: int = MODE_EXACT,
                 worker_lo: int = 0, worker_hi: int | None = None, lib_path: str | None = None):
        self.L = load_library(lib_path)
        self.ctx = None
        n = 5 ** kmer_size if (flags & P.SQ_METH) else 1 << (2 * kmer_size)
        if len(level_mean) != n or len(level_stdv) != n:
            raise ValueError("pore model must have 4^k rows (5^k for the methylation tables)")
        self._model = (CKmer * n)()
        a = np.frombuffer(self._model, dtype=np.float32).reshape(n, 2)
        a[:, 0] = level_mean
        a[:, 1] = level_stdv
        cfg = CCfg(ABI_VERSION, CProfile(*profile.as_tuple()), flags & 0x303d, amp_noise, kmer_size,
                   self._model, seed, num_workers, worker_lo,
                   num_workers if worker_hi is None else worker_hi, device, mode)
        h = C.c_void_p()
        rc = self.L.sqg_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise SqgError(rc, "sqg_create", self.L.sqg_strerror(rc).decode())
        self.ctx = h
        self.num_workers, self.kmer_size, self.flags, self.profile = num_workers, kmer_size, flags, profile
        self.device = device

    def _chk(self, rc, where):
        if rc != 0:
            raise SqgError(rc, where, self.L.sqg_last_error(self.ctx).decode())

    def stage(self, seqs, workers=None) -> Batch:
        """seqs: list of bytes (reads as gen_read returns them)."""
        off = np.zeros(len(seqs) + 1, np.int64)
        if len(seqs):
            off[1:] = np.cumsum([len(s) for s in seqs])
        return self.stage_packed(b"".join(seqs), off, workers)

    def stage_packed(self, blob: bytes, off: np.ndarray, workers=None) -> Batch:
        n = len(off) - 1
        off = np.ascontiguousarray(off, np.int64)
        wk = np.ascontiguousarray(workers, np.int32) if workers is not None else None
        h = C.c_void_p()
        rc = self.L.sqg_batch_stage(self.ctx, n, blob, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                    wk.ctypes.data_as(C.POINTER(C.c_int32)) if wk is not None else None,
                                    C.byref(h))
        self._chk(rc, "sqg_batch_stage")
        return Batch(self, h, n)

    def submit(self, seqs, workers=None) -> Batch:
        return self.stage(seqs, workers).run().wait()

    def load_genome(self, contigs, rlen: int, mode: int = SAMPLE_DNA, trans=None):
        """Keep the reference (list of bytes, as load_ref returned it) on the device for sample()."""
        blob = b"".join(contigs)
        off = np.zeros(len(contigs) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in contigs])
        g = CGenome(len(contigs), C.cast(C.c_char_p(blob), C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), rlen, mode, 0, None, None)
        if trans is not None:
            csum = np.ascontiguousarray(trans[0], np.float32)
            idx = np.ascontiguousarray(trans[1], np.int32)
            g.n_trans = len(csum)
            g.trans_csum = csum.ctypes.data_as(C.POINTER(C.c_float))
            g.trans_idx = idx.ctypes.data_as(C.POINTER(C.c_int32))
        self._chk(self.L.sqg_genome_load(self.ctx, C.byref(g)), "sqg_genome_load")
        self.genome_len = int(off[-1])

    def set_meth(self, contigs, names, meth_freq_path: str):
        """--meth-freq FILE (tab separated: contig, 0-based position of a C, frequency) for the genome loaded with
        load_genome(contigs): the per-base frequency bytes load_meth_freq builds (src/ref.c:291-361)"""
        blob, has = load_meth_freq(contigs, names, meth_freq_path)
        self._chk(self.L.sqg_genome_set_meth(self.ctx, blob.ctypes.data, has.ctypes.data), "sqg_genome_set_meth")

    def load_genome_device(self, d_seqs: int, contig_lens, rlen: int, mode: int = SAMPLE_DNA):
        """The same for a reference that already sits in device memory: d_seqs is the device address of the concatenated
        contigs (e.g. torch_tensor.data_ptr()); it is copied, the caller may free it afterwards."""
        off = np.zeros(len(contig_lens) + 1, np.int64)
        off[1:] = np.cumsum(np.asarray(contig_lens, np.int64))
        g = CGenome(len(contig_lens), C.c_void_p(d_seqs), off.ctypes.data_as(C.POINTER(C.c_int64)), rlen, mode, 0, None, None)
        self._chk(self.L.sqg_genome_load_device(self.ctx, C.byref(g)), "sqg_genome_load_device")
        self.genome_len = int(off[-1])

    def set_range_mode(self, on: bool = True):
        """range sharding (include/sqg.h): this context owns all workers and generates a range of each batch's reads"""
        self._chk(self.L.sqg_set_range_mode(self.ctx, 1 if on else 0), "sqg_set_range_mode")

    def skip_reads(self, seq_lens, workers):
        ln = np.ascontiguousarray(seq_lens, np.int64)
        wk = np.ascontiguousarray(workers, np.int32)
        assert ln.shape == wk.shape
        self._chk(self.L.sqg_skip_reads(self.ctx, len(ln), ln.ctypes.data_as(C.POINTER(C.c_int64)),
                                        wk.ctypes.data_as(C.POINTER(C.c_int32))), "sqg_skip_reads")

    def sample(self, n: int, workers=None, lo: int | None = None, hi: int | None = None) -> Batch:
        """gen_read for n reads on the device + staging; the returned batch carries .sampled (per-read arrays).
        lo/hi (range sharding): all n reads are sampled, reads [lo, hi) are staged."""
        wk = np.ascontiguousarray(workers, np.int32) if workers is not None else None
        wkp = wk.ctypes.data_as(C.POINTER(C.c_int32)) if wk is not None else None
        h = C.c_void_p()
        info = CSample()
        if lo is None and hi is None:
            rc = self.L.sqg_batch_sample(self.ctx, n, wkp, C.byref(h), C.byref(info))
        else:
            lo, hi = (0 if lo is None else lo), (n if hi is None else hi)
            rc = self.L.sqg_batch_sample_range(self.ctx, n, wkp, lo, hi, C.byref(h), C.byref(info))
            n = hi - lo
        self._chk(rc, "sqg_batch_sample")
        b = Batch(self, h, n)
        arr = lambda p, shape, dt: (np.ctypeslib.as_array(p, shape=shape).copy() if n else np.zeros(0, dt))  # noqa: E731
        b.sampled = dict(ref_idx=arr(info.ref_idx, (n,), np.int32), ref_len=arr(info.ref_len, (n,), np.int32),
                         ref_pos=arr(info.ref_pos, (n,), np.int32), rlen=arr(info.rlen, (n,), np.int32),
                         strand=bytes(info.strand[:n]) if n else b"",
                         seq_off=np.ctypeslib.as_array(info.seq_off, shape=(n + 1,)).copy())
        return b

    def new_pileup(self, by="ref", split=(), norm="pa", trim: bool = False, segs=None, lo: int | None = None, hi: int | None = None,
                   outputs=None) -> Pileup:
        """A zeroed pileup for Batch.pileup() (include/sqg_pileup.h): torch tensors [planes, hi - lo] on the context's device -- n (uint32
        bit patterns in an int32 tensor), dwell, dwell_sq, mean_sum, mean_sq, sd_sum (int64; mean and sd in units of 1 / 4096).
        by: "ref" (key: the forward-strand coordinate of the event's k-mer in the loaded genome) or "kmer" (its pore-table row);
        split: any of "strand", "meth": a plane each; segs (by="kmer"): the segments counted, e.g. (3,) (default: the insert);
        [lo, hi): the key window, default the whole loaded genome / all rows.  outputs: the names wanted (default all); the others are None."""
        import torch
        _need(self.L, "sqg_batch_pileup", "sqg_pileup.h", "pileup")
        bv, nm = _enum("pileup", by=by, norm=norm)
        sp = 0
        for name in ((split,) if isinstance(split, (str, int)) else split):
            bit = {"strand": PILEUP_SPLIT_STRAND, "meth": PILEUP_SPLIT_METH}.get(name, name)
            if not isinstance(bit, int):
                raise SqgError(-1, "pileup", f"unknown split {name!r}")
            sp |= bit
        sg = 0
        for q in (() if segs is None else segs):
            sg |= 1 << int(q)
        want = _want(outputs, PILEUP_OUTPUTS, "pileup")
        if lo is None:
            lo = 0
        if hi is None:
            if bv == PILEUP_BY_KMER:
                hi = 5 ** self.kmer_size if (self.flags & P.SQ_METH) else 1 << (2 * self.kmer_size)
            else:
                if getattr(self, "genome_len", None) is None:
                    raise SqgError(-1, "pileup", "by=\"ref\" without hi= needs a loaded genome")
                hi = self.genome_len
        if hi < lo:
            raise SqgError(-1, "pileup", "hi must not be below lo")
        planes = (2 if sp & PILEUP_SPLIT_STRAND else 1) * (2 if sp & PILEUP_SPLIT_METH else 1)
        cfg = CPileupCfg(bv, sp & 0xffffffff, nm, int(trim), sg & 0xffffffff, int(lo), int(hi))
        dev = torch.device("cuda", self.device)
        return Pileup(cfg, planes, **{n: (torch.zeros((planes, hi - lo), dtype=torch.int32 if n == "n" else torch.int64, device=dev) if n in want else None)
                                      for n in PILEUP_OUTPUTS})

    def new_call_freq(self, lo: int | None = None, hi: int | None = None, outputs=None) -> CallFreq:
        """A zeroed called-frequency table for Batch.call(freq=...) (include/sqg_call.h): torch tensors [hi - lo] on the context's device --
        cov, truth, called, meth (uint32 bit patterns in int32 tensors) -- keyed by the forward-strand coordinate of a CpG's C.  [lo, hi):
        default the whole loaded genome.  outputs: the names wanted (default all); the others are None."""
        import torch
        _need(self.L, "sqg_batch_call", "sqg_call.h", "call")
        want = _want(outputs, CALL_FREQ, "call")
        lo = 0 if lo is None else int(lo)
        if hi is None:
            if getattr(self, "genome_len", None) is None:
                raise SqgError(-1, "call", "new_call_freq without hi= needs a loaded genome")
            hi = self.genome_len
        if hi < lo:
            raise SqgError(-1, "call", "hi must not be below lo")
        dev = torch.device("cuda", self.device)
        return CallFreq(lo, int(hi), **{n: (torch.zeros(int(hi) - lo, dtype=torch.int32, device=dev) if n in want else None) for n in CALL_FREQ})

    def map_levels(self):
        """The recommended levels of include/sqg_map.h from the context's own pore model: int32 [4^k] ([5^k] in an SQG_METH context) on the context's
        device, rint(256 * level_mean * digitisation / range) in doubles, clipped to +-2^23.  Made once per context; a binding
        recommendation and not part of the kernel's rule, in the way call_model() is."""
        import torch
        _need(self.L, "sqg_map_track", "sqg_map.h", "map")
        if getattr(self, "_map_levels", None) is None:
            mean = np.frombuffer(self._model, dtype=np.float32).reshape(-1, 2)[:, 0].astype(np.float64)
            lv = np.rint(256.0 * mean * np.float64(self.profile.digitisation) / np.float64(self.profile.range))
            lv = np.nan_to_num(np.clip(lv, -(1 << 23), 1 << 23), nan=0.0).astype(np.int32)
            self._map_levels = torch.from_numpy(lv).to(torch.device("cuda", self.device))
        return self._map_levels

    def new_map_track(self, lo: int | None = None, hi: int | None = None, levels=None, fwd: bool = True, rev: bool = True) -> MapTrack:
        """The level track of the window [lo, hi) of the loaded genome (default: all of it) on both strands (sqg_map_track,
        include/sqg_map.h): a MapTrack for Batch.map().  levels: int32 [4^k] / [5^k] on the context's device, default map_levels().
        fwd=False / rev=False leave that strand out (None)."""
        import torch
        _need(self.L, "sqg_map_track", "sqg_map.h", "map")
        lo = 0 if lo is None else int(lo)
        if hi is None:
            if getattr(self, "genome_len", None) is None:
                raise SqgError(-1, "map", "new_map_track without hi= needs a loaded genome")
            hi = self.genome_len
        hi = int(hi)
        dev = torch.device("cuda", self.device)
        levels = self.map_levels() if levels is None else levels
        rows = 5 ** self.kmer_size if (self.flags & P.SQ_METH) else 1 << (2 * self.kmer_size)
        if not (isinstance(levels, torch.Tensor) and levels.dtype == torch.int32 and levels.device == dev and levels.is_contiguous() and levels.numel() >= rows):
            raise SqgError(-1, "map", f"levels must be a contiguous {torch.int32} tensor of at least {rows} elements on {dev}")
        w = max(hi - lo, 0) if hi - lo <= MAP_MAX_WINDOW else 0      # (the library refuses the window; nothing is allocated for it)
        tr = MapTrack(lo, hi, torch.zeros(w, dtype=torch.int32, device=dev) if fwd else None, torch.zeros(w, dtype=torch.int32, device=dev) if rev else None)
        torch.cuda.synchronize(dev)                         # (the zero fills, before another stream writes the blocks)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None     # noqa: E731
        self._chk(self.L.sqg_map_track(self.ctx, lo, hi, levels.data_ptr(), ptr(tr.fwd), ptr(tr.rev)), "sqg_map_track")
        return tr

    def call_model(self):
        """(w, c): the recommended model tables of include/sqg_call.h from the context's own pore model, int32 tensors [5^k] on the
        context's device: sdc = level_stdv * digitisation / range in doubles, w = clip(rint(2^24 / (2 sdc sdc)), 0, 2^24),
        c = clip(rint(256 ln(sdc)), +-2^20).  Made once per context."""
        import torch
        if getattr(self, "_call_model", None) is None:
            stdv = np.frombuffer(self._model, dtype=np.float32).reshape(-1, 2)[:, 1].astype(np.float64)
            sdc = stdv * np.float64(self.profile.digitisation) / np.float64(self.profile.range)
            with np.errstate(divide="ignore", invalid="ignore"):
                w = np.nan_to_num(np.clip(np.rint(float(1 << 24) / (2.0 * sdc * sdc)), 0, 1 << 24), nan=0.0)
                c = np.nan_to_num(np.clip(np.rint(256.0 * np.log(sdc)), -(1 << 20), 1 << 20), nan=0.0)
            dev = torch.device("cuda", self.device)
            self._call_model = tuple(torch.from_numpy(a.astype(np.int32)).to(dev) for a in (w, c))
        return self._call_model

    def pinned(self, nbytes: int, dtype=np.uint8) -> np.ndarray:
        """A page-locked host array (sqg_host_alloc) for fast sqg_fetch_* destinations; freed with the generator."""
        p = self.L.sqg_host_alloc(nbytes)
        if not p:
            raise MemoryError("sqg_host_alloc")
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        buf = (C.c_uint8 * nbytes).from_address(p)
        return np.frombuffer(buf, dtype=dtype)

    def set_stage_threads(self, n: int) -> int:
        """Host threads that share a batch's per-read libm draws at staging (0: automatic); returns how many the last staging used."""
        rc = self.L.sqg_set_stage_threads(self.ctx, int(n))
        if rc < 0:
            self._chk(rc, "sqg_set_stage_threads")
        return rc

    def set_phase_timing(self, every: int):
        """Phase events (timing()'s milliseconds) on the batches whose run index is a multiple of `every`; 1: all (default), 0: none."""
        self._chk(self.L.sqg_set_phase_timing(self.ctx, int(every)), "sqg_set_phase_timing")

    def timing(self):
        t = CTiming()
        self._chk(self.L.sqg_get_timing(self.ctx, C.byref(t)), "sqg_get_timing")
        return {"dwell_ms": t.dwell_ms, "events_ms": t.events_ms, "samples_ms": t.samples_ms,
                "lean_ms": t.lean_ms, "total_ms": t.total_ms, "fallback_samples": t.fallback_samples,
                "carried_first_pass": bool(t.carried_first_pass), "first_pass_ran_ahead": bool(t.first_pass_ran_ahead)}

    def probe_store_bandwidth(self, nbytes=1 << 30, iters=10) -> float:
        ms = C.c_float()
        self._chk(self.L.sqg_probe_store_bandwidth(self.ctx, nbytes, iters, C.byref(ms)), "sqg_probe_store_bandwidth")
        return nbytes / (ms.value * 1e-3)

    def probe_lds_order(self, workgroups=1024, rounds=16):
        """(mismatches, in_use): the device's LDS atomics against their serial result; whether this context relies on them"""
        bad, used = C.c_uint(), C.c_int()
        self._chk(self.L.sqg_probe_lds_order(self.ctx, workgroups, rounds, C.byref(bad), C.byref(used)), "sqg_probe_lds_order")
        return bad.value, bool(used.value)

    def close(self):
        if self.ctx:
            for p in getattr(self, "_pinned", []):
                self.L.sqg_host_free(p)
            self._pinned = []
            self.L.sqg_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
