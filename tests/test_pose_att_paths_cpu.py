"""The checker of tests/test_pose_att_paths_gpu.py, held to account without a GPU (tests/_pal_stage.py).

(a) Admissibility: an fp32 torch emulation of each stage of csrc/apa_pose_att.hip passes every case of the table --
    every stage inside its bound, every bound below 1 % of max |ref| (`check` asserts both).  The emulation rounds
    where the kernels round but sums in torch's own order, so this shows the bounds admit a correct fp32 kernel for the
    very inputs the GPU test uses.
(b) Seeded errors: the same emulation with one value error in one stage is rejected, and the assertion names that
    stage.  This is the evidence that the GPU test fails on a subtly wrong kernel, without building wrong kernels.
"""
import pytest

from tests import _pal_stage as ps

_CACHE = {}


def _inputs(name):
    """operands and mask of a case, computed once and never written to."""
    if name not in _CACHE:
        c = ps.BY_NAME[name]
        _CACHE.clear()                                   # one case's operands at a time
        _CACHE[name] = (c, ps.make_inputs(c), ps.host_mask(c))
    return _CACHE[name]


@pytest.mark.parametrize('name', [c['name'] for c in ps.CASES])
def test_emulation_is_admitted(name):
    c, I, mask = _inputs(name)
    figs = []
    ps.verify(c, I, mask, ps.emulate(c, I, mask), rec=lambda *a: figs.append(a))
    assert [s for s, _, _ in figs if '[' not in s] == [s for s in ps.STAGES if s not in ('part', 'dA')]
    assert all(r <= 1.0 and b < 0.01 for _, r, b in figs)


# (mutation, case, the stage that must reject it)
SEEDED = [
    ('F_pixel_dropped', 'm5_c260_p65', 'F'),                   # one pixel dropped from one map of F
    ('F_pixel_dropped', 'm1_const_only', 'F'),
    ('logits_slab_left_out', 'm17_parts_n33', 'logits'),       # one classifier slab (the ragged last) left out
    ('logits_slab_left_out', 'm5_c260_p65', 'logits'),
    ('dW_stored', 'm17_parts_n33', 'dW'),                      # dW stored instead of added in the second image block
    ('dPl_stored', 'm4_repeat_c12_acc', 'dPl'),                # dPl stored instead of added
    ('dPl_stored', 'm1_const_only', 'dPl'),
    ('dX0_ignored', 'm4_repeat_c12_acc', 'dX'),                # the given dX ignored under accumulate_dX
    ('dX0_ignored', 'm18_bf16_keep02_acc', 'dX'),
    ('keep_bit_fwd', 'm5_c260_p65', r'part\[\d+\]'),           # one keep bit taken from the neighbouring element
    ('keep_bit_bwd', 'm5_c260_p65', 'dF'),
    ('mean_div_nsel', 'm5_c260_p65', 'F'),                     # the mean map divided by n_sel instead of J
    ('fold_mean_div_nsel', 'm5_c260_p65', 'dPl'),
    ('dA_last_slab_dropped', 'm5_c260_p65', 'dPl'),            # the last (one-lane) slab's dA partial dropped
]


@pytest.mark.parametrize('mut,name,stage', SEEDED, ids=['{}-{}'.format(m, n) for m, n, _ in SEEDED])
def test_seeded_error_is_rejected(mut, name, stage):
    c, I, mask = _inputs(name)
    with pytest.raises(AssertionError, match=r'{}: stage {}:'.format(name, stage)):
        ps.verify(c, I, mask, ps.emulate(c, I, mask, mut))
