"""ctypes glue for the explain half of the test-only probe library (csrc/apa_explain_probe.hip, linked into
libapa_gemm_probe.so): what apa_attn_explain decides before its launches -- the pixel splits, the load form, the wave
geometry of the explain_main_kernel instance, the trips of its channel loop and the groups of its largest block.  Host
only: it loads and answers without a GPU."""
import collections
import ctypes

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp

EXPLAIN_PROBE_VERSION = 1
EXPLAIN_SYMBOLS = ('apa_probe_explain_version', 'apa_probe_explain_plan')

# S, nblk: pixel splits per image and blocks; EPV: elements per load (fp32: 4; bf16: 8, or 4 when C % 8 == 4); PIX, U:
# pixels a wave takes at a time and channel vectors per round (ExplainGeom<T>); per_round = 64 * EPV * U channels and
# the rounds of the channel loop; most: the largest pixel count of a block; groups: its groups of PIX pixels (the four
# waves stride over them); S_m1: the evaluation step's split count, before the LDS-size halving; lds: T * C * 4 bytes
ExplainPlan = collections.namedtuple('ExplainPlan', 'S nblk EPV PIX U per_round rounds most groups S_m1 lds')

_lib = None


def load_explain_probe():
    global _lib
    if _lib is None:
        gp.load_probe()                                   # the library is there, and its GEMM half's version
        lib = ctypes.CDLL(gp.PROBE_PATH)
        lib.apa_probe_explain_version.restype = ctypes.c_int64
        assert lib.apa_probe_explain_version() == EXPLAIN_PROBE_VERSION
        lib.apa_probe_explain_plan.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
        lib.apa_probe_explain_plan.restype = ctypes.c_int
        _lib = lib
    return _lib


def plan(N, P, C, K, T, dtype):
    """ExplainPlan of a shape; dtype 'fp32' / 'bf16'.  A shape apa_attn_explain refuses is an error."""
    out = (ctypes.c_int64 * len(ExplainPlan._fields))()
    code = cof.APA_DTYPE_BF16 if dtype == 'bf16' else cof.APA_DTYPE_F32
    if not load_explain_probe().apa_probe_explain_plan(N, P, C, K, T, code, out):
        raise ValueError('apa_attn_explain refuses N=%d P=%d C=%d K=%d T=%d %s' % (N, P, C, K, T, dtype))
    return ExplainPlan(*(int(v) for v in out))


def form(pl, dtype):
    """the load form of explain_main_kernel<T, EPV, TT>: 'fp32', 'bf16/16B' or 'bf16/8B'"""
    return 'fp32' if dtype == 'fp32' else ('bf16/16B' if pl.EPV == 8 else 'bf16/8B')


def trips(pl):
    """trips of the wave-stride group loop that wave 0 of the largest block makes"""
    return (pl.groups + 3) // 4


def ragged_second_round(pl, C):
    """the channel loop runs a last round (not the first) that C does not fill"""
    return pl.rounds >= 2 and C % pl.per_round != 0
