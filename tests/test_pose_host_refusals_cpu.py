"""The refusals of the three public pose-head entry points (csrc/apa_pose_head.hip), pinned byte for byte, and the
workspace carve of two small shapes by hand.  Every call here is refused on the host before anything is launched, so
no GPU is needed and the operand addresses are fakes that nothing dereferences.  The status code, the whole
apa_last_error text (the entry point's name is part of it) and the ORDER in which the refusals fire for a call that
earns several are the interface: a host-side rewrite of the pose head must leave all three alone."""
import pytest

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
DIMS = dict(N=2, P=49, C=256, Cp=256, J=16, dtype=BF16)

# fake, distinct, 256-byte aligned device addresses
_NAMES = ('X', 'W1', 'b1', 'W2', 'b2', 'Ppre', 'Pl', 'dPl', 'dPpre_ext', 'ext_row', 'ext_col', 'dX', 'dW1', 'db1',
          'dW2', 'db2', 'ws')
FAKE = {n: 0x10000 * (i + 1) for i, n in enumerate(_NAMES)}


def _need(**kw):
    d = dict(DIMS, **kw)
    return int(cof.load_library().apa_pose_head_workspace_bytes(d['N'], d['P'], d['C'], d['Cp'], d['J'], d['dtype']))


def _dims(kw):
    d = dict(DIMS, **{k: v for k, v in kw.items() if k in DIMS})
    return [d[k] for k in ('N', 'P', 'C', 'Cp', 'J', 'dtype')]


def _ptrs(names, kw):
    return [kw.get(n, FAKE[n]) for n in names]


def fwd(**kw):
    lib = cof.load_library()
    rc = lib.apa_pose_head_fwd(*_ptrs(('X', 'W1', 'b1', 'W2', 'b2', 'Ppre', 'Pl', 'ws'), kw),
                               kw.get('ws_bytes', 1 << 40), *_dims(kw), None)
    return rc, lib.apa_last_error()


def bwd(**kw):
    lib = cof.load_library()
    rc = lib.apa_pose_head_bwd(*_ptrs(('X', 'W1', 'W2', 'Ppre', 'dPl', 'dPpre_ext', 'dX'), kw), kw.get('acc', 0),
                               *_ptrs(('dW1', 'db1', 'dW2', 'db2', 'ws'), kw), kw.get('ws_bytes', 1 << 40),
                               *_dims(kw), None)
    return rc, lib.apa_last_error()


def bwd_rank1(**kw):
    lib = cof.load_library()
    rc = lib.apa_pose_head_bwd_rank1ext(*_ptrs(('X', 'W1', 'W2', 'Ppre', 'dPl', 'ext_row', 'ext_col', 'dX'), kw),
                                        kw.get('acc', 0), *_ptrs(('dW1', 'db1', 'dW2', 'db2', 'ws'), kw),
                                        kw.get('ws_bytes', 1 << 40), *_dims(kw), None)
    return rc, lib.apa_last_error()


# ------------------------------------------------------------------------------------------ apa_pose_head_fwd
@pytest.mark.parametrize('name', ('X', 'W1', 'b1', 'W2', 'b2', 'Ppre', 'Pl'))
def test_fwd_null_pointer(name):
    assert fwd(**{name: None}) == (INVALID, b'apa_pose_head_fwd: null pointer or non-positive dimension')


@pytest.mark.parametrize('dim', ('N', 'P', 'C', 'Cp', 'J'))
@pytest.mark.parametrize('value', (0, -3))
def test_fwd_non_positive_dimension(dim, value):
    assert fwd(**{dim: value}) == (INVALID, b'apa_pose_head_fwd: null pointer or non-positive dimension')


def test_fwd_unknown_dtype():
    assert fwd(dtype=7) == (INVALID, b'apa_pose_head_fwd: unknown dtype 7')
    assert fwd(dtype=-1) == (INVALID, b'apa_pose_head_fwd: unknown dtype -1')
    # ... and the null-pointer list comes first
    assert fwd(dtype=7, X=None) == (INVALID, b'apa_pose_head_fwd: null pointer or non-positive dimension')


def test_fwd_workspace_too_small():
    need = _need()
    assert need == 8699904
    assert fwd(ws_bytes=need - 1) == (WORKSPACE, b'apa_pose_head_fwd: workspace too small (%d < %d)' % (need - 1, need))
    assert fwd(ws_bytes=0) == (WORKSPACE, b'apa_pose_head_fwd: workspace too small (0 < %d)' % need)
    # a null workspace is the same refusal, whatever size is claimed for it
    assert fwd(ws=None, ws_bytes=need) == (WORKSPACE, b'apa_pose_head_fwd: workspace too small (%d < %d)' % (need, need))
    # the dtype refusal comes before the workspace one
    assert fwd(dtype=7, ws=None, ws_bytes=0) == (INVALID, b'apa_pose_head_fwd: unknown dtype 7')


# ------------------------------------------------------------------------------------------ apa_pose_head_bwd
@pytest.mark.parametrize('name', ('X', 'W1', 'W2', 'Ppre', 'dX', 'dW1', 'db1', 'dW2', 'db2'))
def test_bwd_null_pointer(name):
    assert bwd(**{name: None}) == (INVALID, b'apa_pose_head_bwd: null pointer or non-positive dimension')


@pytest.mark.parametrize('dim', ('N', 'P', 'C', 'Cp', 'J'))
def test_bwd_non_positive_dimension(dim):
    assert bwd(**{dim: 0}) == (INVALID, b'apa_pose_head_bwd: null pointer or non-positive dimension')


def test_bwd_no_gradient_given():
    assert bwd(dPl=None, dPpre_ext=None) == (
        INVALID, b'apa_pose_head_bwd: neither dPl nor dPpre_ext given (no gradient to propagate)')
    # either one alone passes that check (and is refused further down, here for the workspace)
    assert bwd(dPl=None, ws_bytes=0)[0] == WORKSPACE
    assert bwd(dPpre_ext=None, ws_bytes=0)[0] == WORKSPACE


def test_bwd_j_33():
    assert bwd(J=33) == (UNSUPPORTED, b'apa_pose_head_bwd: J=33 > 32 or Cp=256 > 2048 not built')
    # before the workspace refusal
    assert bwd(J=33, ws=None, ws_bytes=0) == (UNSUPPORTED, b'apa_pose_head_bwd: J=33 > 32 or Cp=256 > 2048 not built')


def test_bwd_cp_2052():
    assert bwd(Cp=2052) == (UNSUPPORTED, b'apa_pose_head_bwd: J=16 > 32 or Cp=2052 > 2048 not built')


def test_bwd_workspace_too_small():
    need = _need()
    assert bwd(ws_bytes=need - 1) == (WORKSPACE, b'apa_pose_head_bwd: workspace too small (%d < %d)' % (need - 1, need))
    assert bwd(ws=None, ws_bytes=need) == (WORKSPACE, b'apa_pose_head_bwd: workspace too small (%d < %d)' % (need, need))
    # an unknown dtype is no refusal of its own in the backward pass; with the workspace missing that is what is said
    need7 = _need(dtype=7)
    assert bwd(dtype=7, ws_bytes=0) == (WORKSPACE, b'apa_pose_head_bwd: workspace too small (0 < %d)' % need7)


def test_bwd_cp_770_with_a_sufficient_workspace_is_the_multiple_of_4_refusal():
    need = _need(Cp=770)
    assert need == 26222080
    for dPpre_ext in (FAKE['dPpre_ext'], None):
        assert bwd(Cp=770, ws_bytes=need, dPpre_ext=dPpre_ext) == (
            UNSUPPORTED, b'apa_pose_head_bwd: Cp=770 must be a multiple of 4')
    assert bwd(Cp=770, ws_bytes=_need(Cp=770, dtype=F32), dtype=F32) == (
        UNSUPPORTED, b'apa_pose_head_bwd: Cp=770 must be a multiple of 4')


def test_bwd_null_workspace_with_cp_770_is_the_workspace_refusal():
    need = _need(Cp=770)
    assert bwd(Cp=770, ws=None, ws_bytes=need) == (
        WORKSPACE, b'apa_pose_head_bwd: workspace too small (%d < %d)' % (need, need))
    assert bwd(Cp=770, ws_bytes=need - 1) == (
        WORKSPACE, b'apa_pose_head_bwd: workspace too small (%d < %d)' % (need - 1, need))


# ------------------------------------------------------------------------------------------ apa_pose_head_bwd_rank1ext
def test_rank1ext_null_ext_row():
    assert bwd_rank1(ext_row=None) == (INVALID, b'apa_pose_head_bwd_rank1ext: null ext_row / ext_col')
    assert bwd_rank1(ext_col=None) == (INVALID, b'apa_pose_head_bwd_rank1ext: null ext_row / ext_col')
    # its own check comes first; everything behind it speaks as apa_pose_head_bwd
    assert bwd_rank1(ext_row=None, X=None) == (INVALID, b'apa_pose_head_bwd_rank1ext: null ext_row / ext_col')
    assert bwd_rank1(X=None) == (INVALID, b'apa_pose_head_bwd: null pointer or non-positive dimension')
    assert bwd_rank1(dPl=None, J=33) == (UNSUPPORTED, b'apa_pose_head_bwd: J=33 > 32 or Cp=256 > 2048 not built')
    need = _need(Cp=770)
    assert bwd_rank1(Cp=770, ws_bytes=need) == (UNSUPPORTED, b'apa_pose_head_bwd: Cp=770 must be a multiple of 4')
    assert bwd_rank1(Cp=770, ws=None, ws_bytes=need) == (
        WORKSPACE, b'apa_pose_head_bwd: workspace too small (%d < %d)' % (need, need))


# ------------------------------------------------------------------------------------------ the workspace carve
def test_pose_plan_of_two_small_shapes_by_hand():
    """[dPpre | partial rows | GEMM split-K scratch | bf16 copy of W1 | loss partials], each region 256-byte aligned.
      (2, 49, 256, 256, 16) bf16: R = 98, 13 chunks of 8 rows
        dPpre    98 x 256 x 2                                            =   50176
        partial  7 blocks of 16 rows x (128 x 32 + 256 + 16 + 256 + 4) x 4 = 129584 -> 129792   (> 13 x 272 x 4)
        GEMM     max(98 x 16, 256 x 16, 256 x 256) x 32 splits x 4       = 8388608
        W1 copy  256 x 256 x 2                                           =  131072
        loss     max(4 blocks x 4, apa_pose_l2_workspace_bytes = 64)     -> 256
      (1, 9, 64, 20, 3) fp32: R = 9, 2 chunks
        dPpre    9 x 20 x 4 = 720 -> 768
        partial  1 block x (20 x 3 + 20 + 3 + 20 + 4) x 4 = 428 -> 512                           (> 2 x 23 x 4)
        GEMM     max(9 x 3, 20 x 3, 64 x 20) x 32 x 4                    = 163840
        W1 copy  64 x 20 x 2                                             = 2560
        loss     -> 256"""
    from tests import _pose_probe as pp
    lib = cof.load_library()
    pl = pp.plan(2, 49, 256, 256, 16, BF16)
    assert [pl[k] for k in pp.PLAN_FIELDS] == [98, 13, 0, 50176, 50176 + 129792, 179968 + 8388608,
                                               8568576 + 131072, 8699648 + 256]
    assert [pl[k] for k in pp.PLAN_FIELDS] == [98, 13, 0, 50176, 179968, 8568576, 8699648, 8699904]
    assert lib.apa_pose_head_workspace_bytes(2, 49, 256, 256, 16, BF16) == 8699904
    pl = pp.plan(1, 9, 64, 20, 3, F32)
    assert [pl[k] for k in pp.PLAN_FIELDS] == [9, 2, 0, 768, 768 + 512, 1280 + 163840, 165120 + 2560, 167680 + 256]
    assert [pl[k] for k in pp.PLAN_FIELDS] == [9, 2, 0, 768, 1280, 165120, 167680, 167936]
    assert lib.apa_pose_head_workspace_bytes(1, 9, 64, 20, 3, F32) == 167936
    assert lib.apa_pose_head_workspace_bytes(0, 9, 64, 20, 3, F32) == 0
