"""The case table of tests/test_fp8_instances_gpu.py -- every instance, lane occupancy and chunk-loop trip count of the
two FP8 streaming kernels (csrc/apa_m1_fp8.hip) -- with the keys each case reaches (tests/test_fp8_instances_cpu.py
asserts the table reaches them all, without a GPU), the cases' inputs and the conditions those inputs must meet.  Test
infrastructure; importable without a GPU.

What a case reaches is computed from the dispatch itself, not from a copy of its rule: NV from apa_probe_m1f_instance
(m1f_vectors_per_lane, which the launchers call), S and the pixels per block from apa_probe_m1_plan (m1_plan), and the
per-wave chunk counts from the kernels' own two lines

    npw    = p_begin + wave < p_end ? (p_end - p_begin - wave + 3) / 4 : 0        (this wave's pixels)
    nchunk = (npw + PIX - 1) / PIX                                                 PIX = 4 / 2 / 1 / 1 for NV = 1 / 2 / 4 / 8

The chunk loop `for (ch = 0; ch < nchunk; ch += 2) for u in 0, 1` is double-buffered: trip (ch, u) consumes ring slot u
and prefetches chunk ch + u + 1 into slot u ^ 1.  nchunk = 0 never enters it, 1 and 2 stay in the first outer trip, an
odd nchunk >= 3 leaves through the `u == 1` break of a later trip, an even one >= 4 through the loop condition; from
the second outer trip on slot 0 holds what the u == 1 prefetch fetched.

Inputs as in tests/test_fp8_features_gpu.py: relu(randn) times a per-pixel scale, per-image magnitudes 1 / 37 / 1e-3
(a wrong or swapped scale[n] cannot pass), positive-mean weights, and for relu a bias that gates the unit-magnitude
images both ways.  They are drawn on the CPU from the case's seed -- a gathered case draws only its T = 7 cache images,
whatever its N -- so that the conditions below can be checked where there is no GPU; the float64 reference of the
N-image batch is formed where the test runs."""
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _m1_probe as mp

T = 7                                   # images in the cache of a gathered case
KEEP, SEED, OFFSET = 0.5, 1234, 7
MAGNITUDES = (1.0, 37.0, 1e-3)          # image n of the source (batch or cache): MAGNITUDES[n % 3]
PIX = {1: 4, 2: 2, 4: 1, 8: 1}          # apa_m1_fp8.hip pix_per_chunk
NARROW = {1: 16, 2: 1040, 4: 2064, 8: 4112}     # the narrowest width of an instance: the last lane row is ragged
WIDE = {1: 1024, 2: 2048, 4: 4096, 8: 8192}     # the widest: every lane active
F32 = cof.APA_DTYPE_F32


def case(N, P, C, K, act, train, gathered, reseed=0, chains=False):
    """chains: the float64 bounds use the kernel's own longest addition chains (kernel_chains) instead of C and P."""
    name = 'n%d_p%d_c%d_k%d_%s_%s_%s' % (N, P, C, K, act, 'train' if train else 'eval', 'gathered' if gathered else 'plain')
    return dict(name=name, N=N, P=P, C=C, K=K, act=act, train=train, gathered=gathered, reseed=reseed, chains=chains)


# (N, P) -> S, chunk counts: (2, 2) -> 1, {0, 1}; (5, 49) -> 12 (blocks of 4 / 5), {1, 2} at PIX = 1; (171, 49) -> 3
# (blocks of 16 / 16 / 17), {1, 2} / {2, 3} at PIX = 4 / 2; (342, 33) -> 1, {4, 5} at PIX = 2; (342, 49) -> 1, {3, 4} at
# PIX = 4; (128, 49) -> 4 (blocks of 12 / 12 / 12 / 13), {3, 4} at PIX = 1.  The large-N cases are gathered ones.
# Every case meets the 1 % rule with the model's default chain lengths (C and P); from C = 4096 on, where those are two
# orders of magnitude above the kernels' own, the bounds are drawn from kernel_chains instead.
CASES = [
    # ---- NV = 1 (C <= 1024, PIX = 4)
    case(2, 2, 16, 20, 'id', False, False),
    case(5, 49, 16, 20, 'relu', True, False),
    case(171, 49, 1024, 20, 'relu', True, True),
    case(342, 49, 1024, 20, 'id', False, True),
    # ---- NV = 2 (C <= 2048, PIX = 2)
    case(2, 2, 1040, 20, 'relu', True, False),
    case(5, 49, 2048, 393, 'id', False, False),
    case(171, 49, 2048, 20, 'id', False, True),
    case(342, 33, 1040, 20, 'relu', True, True),
    # ---- NV = 4 (C <= 4096, PIX = 1)
    case(2, 2, 2064, 20, 'id', True, False),
    case(5, 49, 4096, 393, 'relu', False, False, chains=True),
    case(5, 49, 2064, 20, 'id', False, True),
    case(128, 49, 4096, 20, 'relu', True, True, chains=True),
    # ---- NV = 8 (C <= 8192, PIX = 1)
    case(2, 2, 4112, 393, 'relu', True, False, chains=True),
    case(5, 49, 8192, 20, 'id', False, False, chains=True),
    case(5, 49, 4112, 20, 'relu', False, True, chains=True),
    case(128, 49, 8192, 393, 'relu', True, True, chains=True),
]


def seed_of(c):
    return 4000 + c['N'] + 3 * c['P'] + c['C'] + 7 * c['K'] + len(c['act']) + 2 * c['train'] + c['gathered'] + \
        1000 * c['reseed']


# ------------------------------------------------------------------------------------------ what a case reaches
def blocks(c):
    """(S, [(p_begin, p_end)] of the S blocks of an image): m1_plan's S, the kernels' block bounds."""
    S = mp.plan(c['N'], c['P'], c['C'], c['C'], c['K'])[0]
    return S, [(s * c['P'] // S, (s + 1) * c['P'] // S) for s in range(S)]


def trip_counts(c):
    """{nchunk} over the S blocks' four waves, and the largest npw."""
    pix = PIX[mp.fp8_instance(c['C'])]
    out, most = set(), 0
    for b, e in blocks(c)[1]:
        for wave in range(4):
            npw = (e - b - wave + 3) // 4 if b + wave < e else 0
            most = max(most, npw)
            out.add((npw + pix - 1) // pix)
    return out, most


def trip_class(n):
    return n if n <= 2 else ('odd>=3' if n % 2 else 'even>=4')


def routes(c):
    """(logits, head) of apa_m1.hip m1_forward / m1_backward for a separate forward and backward call with 16-byte
    aligned buffers, from the library's own predicates: the partial-logits product or the split-K one; the head
    kernel (tiles for N > 32 and at most 7 k-tile groups, else rows), the small-K kernel, or two split-K products."""
    sup = mp.support(c['N'], c['C'], c['K'], F32)
    logits = 'logits2' if sup & mp.SUP_LOGITS2 else 'sgemm'
    if not sup & mp.SUP_SMALL:
        return logits, 'sgemm'
    if not sup & mp.SUP_HEAD:
        return logits, 'small'
    ug = ((c['K'] + 15) // 16 + 3) // 4
    return logits, 'tiles' if c['N'] > 32 and ug <= 7 else 'rows'


def reached(c):
    """the keys of the reach table this case reaches"""
    nv = mp.fp8_instance(c['C'])
    assert nv in PIX, (c['name'], nv)
    S = blocks(c)[0]
    keys = {('instance', nv, c['train'], c['gathered'])}
    if c['C'] == NARROW[nv]:
        keys.add(('lanes', nv, 'ragged'))
    if c['C'] == WIDE[nv]:
        keys.add(('lanes', nv, 'full'))
    keys |= {('trips', nv, trip_class(n)) for n in trip_counts(c)[0]}
    if S == 1:
        keys.add(('split', nv, 'S=1'))
    elif c['P'] % S:
        keys.add(('split', nv, 'S>1, P%S!=0'))
    keys.add(('head', nv, c['K']))
    return keys


REQUIRED = set()
for _nv in (1, 2, 4, 8):
    REQUIRED |= {('instance', _nv, tr, ga) for tr in (False, True) for ga in (False, True)}
    REQUIRED |= {('lanes', _nv, 'ragged'), ('lanes', _nv, 'full')}
    REQUIRED |= {('trips', _nv, t) for t in (0, 1, 2, 'odd>=3', 'even>=4')}
    REQUIRED |= {('split', _nv, 'S=1'), ('split', _nv, 'S>1, P%S!=0')}
REQUIRED |= {('head', nv, K) for nv in (4, 8) for K in (20, 393)}


def reach_table(cases=None):
    """{key: [names of the cases that reach it]}"""
    table = {}
    for c in (CASES if cases is None else cases):
        for k in reached(c):
            table.setdefault(k, []).append(c['name'])
    return table


# ------------------------------------------------------------------------------------------ the kernels' chains
def kernel_chains(c):
    """The longest chains of fp32 additions in apa_m1_fp8.hip, for the bounds of tests/_m1_probe.py (a contraction
    accumulated over L terms: C_ACC (L + 8) 2^-24 of the summed magnitudes):
      * a pixel's dot product with wa (forward) or dz (backward): a lane runs two interleaved accumulators d0 / d1 over
        its NV vectors of 16 codes, 8 NV fused multiply-adds each; d0 + d1 is one addition, wave_sum six shuffle
        levels, and one more fused multiply-add applies the image's scale and adds the bias (backward: G . bt)
        -> 8 NV + 8;
      * a pooled sum over the pixels (pacc, pstat; the model's L for zsave and abar): a wave accumulates its own pixels,
        at most ceil(pixels per block / 4), merge_waves adds the four waves' rows in three additions, and the partial
        merge behind the pass adds the image's S blocks -> ceil(ppb / 4) + 3 + S;
      * a logit's contraction over the channels: m1_logits2 sums 64-channel chunks (four of them inside a block for
        N >= 128) and then their partials, sgemm_small m1_plan's lsplits slices and then the slices
        (tests/_rank_reference.logits_chain) -> at most max(256 + C / 64, ceil(C / ls) + ls)."""
    nv = mp.fp8_instance(c['C'])
    S, ppb, _, ls = mp.plan(c['N'], c['P'], c['C'], c['C'], c['K'])
    assert trip_counts(c)[1] == (ppb + 3) // 4
    C = c['C']
    return dict(dot=8 * nv + 8, pool=(ppb + 3) // 4 + 3 + S, logits=max(256 + C // 64, (C + ls - 1) // ls + ls))


# ------------------------------------------------------------------------------------------ inputs
def index_of(c):
    """a gathered case's image ids: the cache's last image first, a repeated id, unordered, every image used"""
    if not c['gathered']:
        return None
    g = torch.Generator().manual_seed(seed_of(c) + 1)
    idx = torch.randint(0, T, (c['N'],), generator=g)
    head = torch.tensor([T - 1, 0, T - 1, 3, 1][:c['N']])
    idx[:head.numel()] = head
    return idx.to(torch.int32)


def model_case(c):
    """the case as tests/test_m1_paths_gpu.py's reference functions read it"""
    return dict(name=c['name'], N=c['N'], P=c['P'], C=c['C'], K=c['K'], J=0, Ca=None, act=c['act'], train=c['train'],
                keep=KEEP, rank1=False, relu_in=False, dt=cof.APA_DTYPE_FP8_E4M3, entry='sep',
                chains=kernel_chains(c) if c['chains'] else None)


def inputs(c, dev, batch=True):
    """-> dict: f8 (the Fp8Features the kernels read: the N-image batch, or the T-image cache), index (int32 on dev, or
    None), src (int64 [N]: the source image of batch position n), X / Xatt (float64 [N,P,C] on dev: scale * decode(code),
    exact), Wa [C], ba [1], Wt [C,K], bt [K], G [N,K] on dev.  Drawn on the CPU by the case's seed, quantised on dev
    (the device's encoder is the CPU rule bit for bit: tests/test_fp8_features_gpu.py).  batch=False: X / Xatt stay the
    source images [n_img,P,C] (a gathered case: the cache's T), for what can be said per image."""
    N, P, C, K = c['N'], c['P'], c['C'], c['K']
    g = torch.Generator().manual_seed(seed_of(c))
    u = lambda *s: torch.rand(s, generator=g) * 1.25 - 0.25
    n_img = T if c['gathered'] else N
    mag = torch.tensor([MAGNITUDES[n % 3] for n in range(n_img)]).view(n_img, 1, 1)
    rows = 0.25 + 1.5 * torch.rand((n_img, P, 1), generator=g)
    img = torch.relu(torch.randn(n_img, P, C, generator=g)) * rows * mag
    f8, status = cof.quantize_features(img.to(dev))
    assert status.tolist() == [0] * n_img
    X64 = f8.codes.to(torch.float32).double() * f8.scale.double().view(n_img, 1, 1)
    Wa = u(C) * (4.0 / C)
    if c['act'] == 'relu':      # the unit-magnitude images gate both ways around their mean pixel
        unit = [n for n in range(n_img) if n % 3 == 0]
        ba = -(X64[unit].float().cpu().mean(dim=(0, 1)) @ Wa).reshape(1)
    else:
        ba = u(1) * 0.1
    index = index_of(c)
    src = torch.arange(N) if index is None else index.long()
    X = X64 if index is None or not batch else X64[src.to(dev)]
    return dict(f8=f8, index=None if index is None else index.to(dev), src=src, X=X, Xatt=X, Wa=Wa.to(dev),
                ba=ba.to(dev), Wt=(u(C, K) / C ** 0.5).to(dev), bt=(u(K) * 0.1).to(dev), G=(u(N, K) / N).to(dev),
                Xext=None)


# ------------------------------------------------------------------------------------------ conditions on the inputs
def one_percent_rule(b, what, ambiguous=None):
    """tests/_m1_probe.check's own condition on a bound, by itself: below 1 % of max |ref|"""
    keep = torch.ones_like(b.ref, dtype=torch.bool) if ambiguous is None else ~ambiguous.expand_as(b.ref)
    scale, worst = float(b.ref.abs()[keep].max()), float(b.err[keep].max())
    assert worst < 0.01 * scale, '{}: bound {:.3g} is not below 1 % of max |ref| {:.3g}'.format(what, worst, scale)
    return worst / scale


def gate_condition(c, inp, att_ref, amb):
    """relu: at most 3 % of the N P gates within their bound of zero; between 10 % and 90 % of the gates of the
    unit-magnitude images open.  att_ref / amb: [N,P] of the batch.  -> (excluded, open on the unit-magnitude images)"""
    if c['act'] != 'relu':
        return 0.0, None
    excl = float(amb.double().mean())
    unit = (inp['src'] % 3 == 0).to(att_ref.device)
    opn = float((att_ref[unit] > 0).double().mean())
    assert excl <= 0.03, '{}: {:.2%} of the relu gates lie within their bound of zero'.format(c['name'], excl)
    assert 0.10 <= opn <= 0.90, '{}: {:.1%} of the unit-magnitude gates are open'.format(c['name'], opn)
    return excl, opn


def check_conditions(c, inp, mask, forward_ref, backward_ref):
    """Every condition of a case, from its inputs alone (the backward bounds on the REFERENCE's own forward values,
    where the test later puts the kernel's): the gate condition, then the 1 % rule on every output's bound.
    forward_ref / backward_ref: tests/test_m1_paths_gpu.py's.  -> (forward reference, ambiguous gates, figures)"""
    mc = model_case(c)
    ref_f, amb = forward_ref(mc, inp, mask)
    figures = dict(gates=gate_condition(c, inp, ref_f['att'].ref, amb))
    figures['att'] = one_percent_rule(ref_f['att'], 'att', amb)
    for k in ('zsave', 'abar', 'logits'):
        figures[k] = one_percent_rule(ref_f[k], k)
    stand_in = dict(att=ref_f['att'].ref, zsave=ref_f['zsave'].ref, abar=ref_f['abar'].ref, G=inp['G'])
    ref_b = backward_ref(mc, inp, stand_in, mask)
    for k in ('dWa', 'dba', 'dWt', 'dbt'):
        figures[k] = one_percent_rule(ref_b[k], k)
    return ref_f, amb, figures
