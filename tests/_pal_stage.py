"""Stage-by-stage float64 references, error bounds and an fp32 emulation of the pose-heatmap attention head
(csrc/apa_pose_att.hip).  Test infrastructure shared by tests/test_pose_att_paths_gpu.py (the six kernels on the GPU)
and tests/test_pose_att_paths_cpu.py (the emulation, and seeded errors, through the same checker).

The kernel instance is a pure function of (M, dtype, accumulate_dX), which a case fixes, and every intermediate lives
in caller-owned memory (`layout` transcribes pal_plan).  Each stage is held, element by element, to float64 computed
from THE TENSORS THAT STAGE'S KERNEL READ -- the stored outputs of the earlier stages, not their float64 values:

  stage    float64 from                               bound (Bnd / contract of tests/_m1_probe.py)
  F        X, Pl                                      contract(L = P) .scale(1/P) .rounded(2): the float 1/P and the
                                                      product; the mean map = sum_j Pl / J carries
                                                      C_ACC (J + 8) 2^-24 mean_j |Pl|
  part[s]  own F, mask, rows of W in slab s           Fd = F mask / keep .rounded(2) (the float 1/keep and the product;
                                                      eval: Fd = F exactly); contract(L = rows of the slab)
  logits   own part, b                                C_ACC (nslab + 8) 2^-24 sum_s |part|, + b, one rounding
  dF       G, W, mask                                 contract(L = K), times mask / keep .rounded(2): exactly 0 where
                                                      the mask is 0; eval: no factor, no rounding
  dW       own F, mask, G                             contract(L = N) of Fd
  db       G                                          contract(L = N)
  dX       own dF, Pl, the given dX (accumulate)      g = dF / P .rounded(2); contract(L = M); + dX0 .rounded();
                                                      a bf16 store adds 2^-8 |ref|
  dA[s]    X, own dF, channels of slab s              contract(L = 256) of X and g
  dPl      the given dPl, own dA                      slab sum C_ACC (nslab + 8) 2^-24 sum_s |dA|; the mean map's share
                                                      / J .rounded(2); the fold and the add onto dPl0:
                                                      C_ACC (M + 8) 2^-24 mag on the elements a map reaches, 0 elsewhere
                                                      (M = 1: dPl == dPl0 exactly)

keep is the float the kernels receive (float32(keep_prob)).  The mask is exact: cof.dropout_mask on the GPU,
tests/golden/apa_keep_mask.py (its numpy twin) without one.

Inputs (positive-mean recipe, as in the other path tests, so that every bound stays below 1 % of max |ref|, which
`check` asserts): X = relu(U(-0.25, 1)) * pixel scale U(0.5, 1.5), rounded to bf16 for bf16 features; Pl = U(-0.25, 1);
W = U(-0.25, 1) / (M C); b = 0.1 N(0, 1); G = U(-0.25, 1) / N; dPl0 = 0.01 U(-0.25, 1); dX0 = 0.01 U(-0.25, 1).  They
are drawn on the host from a generator seeded by the case's name, so both test files see the same values.
"""
import zlib

import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests._m1_probe import Bnd, C_ACC, EPS32, check, contract, tolerance

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
TDT = {F32: torch.float32, BF16: torch.bfloat16}
SEED, OFFSET = 1234, 5
SLAB = 256                        # PAL_SLAB = CLS_ROWS (csrc/apa_pose_att.hip)
IMG_BLOCK = 32                    # images per pass of the two classifier kernels
STAGES = ('F', 'part', 'logits', 'dF', 'dW', 'db', 'dX', 'dA', 'dPl')


def case(name, N, P, C, J, K, sel, avged, dt=F32, keep=None, acc=False):
    """keep=None: eval; keep=p: APA_FLAG_TRAIN with keep_prob p; acc: accumulate_dX."""
    sel = [int(j) for j in sel]
    return dict(name=name, N=N, P=P, C=C, J=J, K=K, sel=sel, avged=bool(avged), dt=dt, train=keep is not None,
                keep=1.0 if keep is None else keep, acc=acc, M=len(sel) + (1 if avged else 0) + 1)


# The smallest shapes at which each edge exists.  MT instance: M <= 4 / 8 / 17 / 32.
CASES = [
    # M = 1; R = 4 (one MFMA k-step, 15 of 16 rows idle); P = 1 (7 waves idle); dPl untouched
    case('m1_const_only', 1, 1, 4, 1, 1, [], False),
    # the mean map only; one slab with its last lane idle; P is exactly one chunk
    case('m2_avg_only_c252', 3, 64, 252, 16, 51, [], True),
    # MT = 4 upper edge; a repeated part (the fold adds two maps into one j); J = 13; P = 9 (wave 0 owns two pixels);
    # K = 17 (second tile has one column); R = 48
    case('m4_repeat_c12_acc', 2, 9, 12, 13, 17, [3, 3, 0], False, keep=0.5, acc=True),
    # the same in bf16: at these small dimensions the maps' share of dX is two orders of magnitude above the bf16
    # rounding of the sum, which at the shipped dimensions of m18_bf16_keep02_acc is as large as the share itself
    case('m4_bf16_repeat_c12_acc', 2, 9, 12, 13, 17, [3, 3, 0], False, dt=BF16, keep=0.5, acc=True),
    # J = 1: part, mean and repeat read the same column
    case('j1_all_maps_equal', 2, 5, 4, 1, 7, [0, 0], True, keep=0.5),
    # MT = 8 lower edge; second slab has one live lane; second pixel chunk has one pixel; N = 16, K = 16 exact tiles
    case('m5_c260_p65', 16, 65, 260, 16, 16, [0, 5, 9], True, keep=0.5),
    # MT = 8 upper edge; two live lanes per wave; image 16 alone in the upper MFMA half; K = 15
    case('m8_bf16_c8_n17', 17, 25, 8, 16, 15, [1, 2, 4, 7, 11, 13], True, dt=BF16),
    # MT = 17 lower edge; KT = 9 (wave 0 takes a second tile of one column); four pixel chunks, the last of 33
    case('m9_bf16_k129', 17, 225, 256, 16, 129, [15] * 7, True, dt=BF16, keep=0.5),
    # the shipped M = 17; N = 33 (second 32-image block of one image: part rewritten per block, dW read-modify-write);
    # three slabs; KT = 25
    case('m17_parts_n33', 33, 49, 516, 16, 393, range(16), False, keep=0.5),
    # MT = 32 lower edge; the shipped P, K and keep; bf16 accumulate with a one-lane slab
    case('m18_bf16_keep02_acc', 40, 196, 260, 16, 393, range(16), True, dt=BF16, keep=0.2, acc=True),
    # M = 32 and K = 480, both maxima (61.6 KB of LDS in pal_cls_bwd_kernel, 65 classifier slabs)
    case('m32_k480', 33, 65, 516, 16, 480, list(range(16)) + list(range(14)), True, keep=0.5),
]
BY_NAME = {c['name']: c for c in CASES}


def layout(N, P, C, M, K):
    """pal_plan, transcribed: byte offsets / element counts of the workspace stages and the total."""
    up = lambda x: (x + 255) // 256 * 256
    R = M * C
    nslab_cls, nslab_pool = (R + SLAB - 1) // SLAB, (C + SLAB - 1) // SLAB
    fwd = up(4 * nslab_cls * N * K)
    dA_off = up(4 * N * R)
    bwd = dA_off + up(4 * nslab_pool * N * P * M)
    return dict(R=R, nslab_cls=nslab_cls, nslab_pool=nslab_pool, part_off=0, part_n=nslab_cls * N * K, dF_off=0,
                dF_n=N * R, dA_off=dA_off, dA_n=nslab_pool * N * P * M, total=max(fwd, bwd))


def make_inputs(c):
    """The case's operands in the dtypes the kernels read, on the host."""
    N, P, C, J, K, M = c['N'], c['P'], c['C'], c['J'], c['K'], c['M']
    tdt = TDT[c['dt']]
    gen = torch.Generator()
    gen.manual_seed(zlib.crc32(c['name'].encode()))
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    ro = lambda *s: rnd(*s) * 1.25 - 0.25
    I = {}
    I['X'] = (torch.relu(ro(N, P, C)) * (0.5 + rnd(N, P, 1))).to(tdt)
    I['Pl'] = ro(N, P, J).float()
    I['W'] = (ro(M * C, K) / (M * C)).float()
    I['b'] = (0.1 * torch.randn(K, generator=gen, dtype=torch.float64)).float()
    I['G'] = (ro(N, K) / N).float()
    I['dPl0'] = (0.01 * ro(N, P, J)).float()
    I['dX0'] = (0.01 * ro(N, P, C)).to(tdt)
    assert bool(I['dPl0'].ne(0).all()) and bool(I['dX0'].ne(0).all())
    return I


def host_mask(c):
    """The {0,1} keep mask over F's flat index, from the numpy twin of the library's hash (None in eval)."""
    if not c['train']:
        return None
    from tests.golden import apa_keep_mask as km
    return torch.from_numpy(km.keep_mask((c['N'], c['M'] * c['C']), c['keep'], SEED, OFFSET).copy())


# ------------------------------------------------------------------------------------------ float64 stages
def _sub(b, idx):
    return Bnd(b.ref[idx], b.err[idx])


class Stages:
    """The float64 reference of every stage of one case.  X, Pl, W, b, G, dPl0, dX0: the operands as the kernels read
    them (any float dtype, one device); mask: {0,1} [N, M*C] or None."""

    def __init__(self, c, I, mask):
        self.c = c
        d = lambda t: t.double()
        self.X, self.Pl, self.W, self.b, self.G = d(I['X']), d(I['Pl']), d(I['W']), d(I['b']), d(I['G'])
        self.dPl0, self.dX0 = d(I['dPl0']), d(I['dX0'])
        self.mask = None if mask is None else mask.to(self.X.device).double().reshape(c['N'], c['M'] * c['C'])
        assert (self.mask is not None) == c['train']
        self.keep = float(torch.tensor(c['keep'], dtype=torch.float32))
        self._A = None

    def maps(self):
        """A [N,P,M]: the selected parts (exact), their mean over all J parts, the constant map (exact)."""
        if self._A is None:
            c, Pl = self.c, self.Pl
            zero = torch.zeros_like(Pl[..., 0])
            cols, errs = [Pl[..., j] for j in c['sel']], [zero] * len(c['sel'])
            if c['avged']:
                cols.append(Pl.sum(-1) / c['J'])
                errs.append(C_ACC * (c['J'] + 8) * EPS32 * Pl.abs().mean(-1))
            cols.append(torch.ones_like(zero))
            errs.append(zero)
            self._A = Bnd(torch.stack(cols, -1), torch.stack(errs, -1))
        return self._A

    def _dropped(self, F):
        """Fd = F * mask / keep: two roundings under APA_FLAG_TRAIN (0 stays 0), F itself in eval."""
        if self.mask is None:
            return Bnd(F)
        return Bnd(F * self.mask / self.keep).rounded(2)

    def F(self):
        c = self.c
        f = contract('npm,npc->nmc', self.maps(), Bnd(self.X), c['P']).scale(1.0 / c['P']).rounded(2)
        return Bnd(f.ref.reshape(c['N'], -1), f.err.reshape(c['N'], -1))

    def part(self, F_own, s):
        R = self.c['M'] * self.c['C']
        rows = slice(s * SLAB, min(R, (s + 1) * SLAB))
        Fd = self._dropped(F_own.double())
        return contract('nr,rk->nk', _sub(Fd, (slice(None), rows)), Bnd(self.W[rows]), rows.stop - rows.start)

    def logits(self, part_own):
        p = part_own.double()
        s = Bnd(p.sum(0), C_ACC * (p.shape[0] + 8) * EPS32 * p.abs().sum(0))
        return (s + Bnd(self.b.expand_as(s.ref))).rounded()

    def dF(self):
        d = contract('nk,rk->nr', Bnd(self.G), Bnd(self.W), self.c['K'])
        if self.mask is None:
            return d
        f = self.mask / self.keep
        return Bnd(d.ref * f, d.err * f).rounded(2)

    def dW(self, F_own):
        return contract('nr,nk->rk', self._dropped(F_own.double()), Bnd(self.G), self.c['N'])

    def db(self):
        return contract('nk,n->k', Bnd(self.G), Bnd(torch.ones_like(self.G[:, 0])), self.c['N'])

    def _g(self, dF_own):
        c = self.c
        return Bnd(dF_own.double().reshape(c['N'], c['M'], c['C']) / c['P']).rounded(2)

    def dX(self, dF_own):
        d = contract('npm,nmc->npc', self.maps(), self._g(dF_own), self.c['M'])
        if self.c['acc']:
            d = (d + Bnd(self.dX0)).rounded()
        return d

    def dA(self, dF_own, s):
        cs = slice(s * SLAB, min(self.c['C'], (s + 1) * SLAB))
        g = self._g(dF_own)
        return contract('npc,nmc->npm', Bnd(self.X[..., cs]), _sub(g, (Ellipsis, cs)), SLAB)

    def dPl(self, dA_own):
        c = self.c
        nsel, J = len(c['sel']), c['J']
        if nsel + (1 if c['avged'] else 0) == 0:
            return Bnd(self.dPl0.clone())                          # the constant map's share is dropped: exact
        a = dA_own.double()
        d = Bnd(a.sum(0), C_ACC * (a.shape[0] + 8) * EPS32 * a.abs().sum(0))
        ref, mag = self.dPl0.clone(), self.dPl0.abs()
        err = torch.zeros_like(ref)
        hit = torch.zeros(J, dtype=torch.bool, device=ref.device)
        for m, j in enumerate(c['sel']):
            ref[..., j] += d.ref[..., m]
            mag[..., j] += d.ref[..., m].abs() + d.err[..., m]
            err[..., j] += d.err[..., m]
            hit[j] = True
        if c['avged']:
            t = _sub(d, (Ellipsis, nsel)).scale(1.0 / J).rounded(2)
            ref += t.ref[..., None]
            mag += (t.ref.abs() + t.err)[..., None]
            err += t.err[..., None]
            hit[:] = True
        err = err + C_ACC * (c['M'] + 8) * EPS32 * mag
        return Bnd(ref, torch.where(hit.expand_as(err), err, torch.zeros_like(err)))


def figures(got, b, bf16=False):
    """(max |got - ref| / tolerance, max bound / max |ref|) of one stage, for the profile note."""
    g = got.double().reshape(b.ref.shape)
    tol = tolerance(b, bf16)
    nz = tol > 0
    r = float(((g - b.ref).abs()[nz] / tol[nz]).max()) if bool(nz.any()) else 0.0
    if bool(((g - b.ref).abs()[~nz] > 0).any()):
        r = float('inf')
    top = float(b.ref.abs().max())
    return r, (float(b.err.max()) / top if top > 0 else 0.0)


def verify(c, I, mask, obs, rec=None):
    """Every stage of `obs` (what the kernels, or the emulation, stored: F [N,R], part [nslab,N,K], logits [N,K],
    dF [N,R], dW [R,K], db [K], dX [N,P,C], dA [nslab,N,P,M], dPl [N,P,J]) against float64, in the order of STAGES.
    An assertion names the case and the stage: '<case>: stage <stage>: ...'.  rec(stage, ratio, bound_over_ref)
    receives the figures before each assertion."""
    st = Stages(c, I, mask)
    bf = c['dt'] == BF16
    lay = layout(c['N'], c['P'], c['C'], c['M'], c['K'])
    assert obs['part'].shape[0] == lay['nslab_cls'] and obs['dA'].shape[0] == lay['nslab_pool']

    def chk(got, b, stage, **kw):
        if rec is not None:
            rec(stage, *figures(got, b, kw.get('bf16', False)))
        check(got, b, '{}: stage {}'.format(c['name'], stage), **kw)

    chk(obs['F'], st.F(), 'F')
    for s in range(lay['nslab_cls']):
        chk(obs['part'][s], st.part(obs['F'], s), 'part[{}]'.format(s))
    chk(obs['logits'], st.logits(obs['part']), 'logits')
    chk(obs['dF'], st.dF(), 'dF')
    chk(obs['dW'], st.dW(obs['F']), 'dW')
    chk(obs['db'], st.db(), 'db')
    chk(obs['dX'], st.dX(obs['dF']), 'dX', bf16=bf)
    for s in range(lay['nslab_pool']):
        chk(obs['dA'][s], st.dA(obs['dF'], s), 'dA[{}]'.format(s))
    chk(obs['dPl'], st.dPl(obs['dA']), 'dPl')
    if c['M'] == 1:
        same = torch.equal(obs['dPl'].reshape(-1).cpu(), I['dPl0'].reshape(-1).cpu())
        assert same, '{}: stage dPl: M = 1 must leave dPl as given, bit for bit'.format(c['name'])


# ------------------------------------------------------------------------------------------ fp32 emulation
MUTATIONS = ('F_pixel_dropped', 'logits_slab_left_out', 'dW_stored', 'dPl_stored', 'dX0_ignored', 'keep_bit_fwd',
             'keep_bit_bwd', 'mean_div_nsel', 'fold_mean_div_nsel', 'dA_last_slab_dropped')


def _neighbour_bit(mask):
    """the mask with one keep bit taken from the neighbouring element (the first pair that differs)."""
    flat = mask.reshape(-1).clone()
    pair = flat.view(-1, 2)
    i = int((pair[:, 0] != pair[:, 1]).nonzero()[0])
    flat[2 * i] = flat[2 * i + 1]
    return flat.view_as(mask)


def emulate(c, I, mask, mut=None):
    """Each stage in plain fp32 torch, reading the emulation's own earlier outputs as the kernels read theirs.
    `mut`: one of MUTATIONS, a value error seeded into one stage."""
    assert mut is None or mut in MUTATIONS
    N, P, C, J, K, M, sel = c['N'], c['P'], c['C'], c['J'], c['K'], c['M'], c['sel']
    R, nsel = M * C, len(c['sel'])
    f32 = torch.float32
    X, Pl, W, b, G = I['X'].float(), I['Pl'], I['W'], I['b'], I['G']
    one = torch.ones((), dtype=f32)
    invP, invJ = one / P, one / J
    cols = [Pl[..., j] for j in sel]
    if c['avged']:
        cols.append(Pl.sum(-1) * (one / nsel if mut == 'mean_div_nsel' else invJ))
    cols.append(torch.ones_like(Pl[..., 0]))
    A = torch.stack(cols, -1)
    Af = A
    if mut == 'F_pixel_dropped':
        Af = A.clone()
        Af[N - 1, P - 1, 0] = 0.0
    F = (torch.einsum('npm,npc->nmc', Af, X) * invP).reshape(N, R)
    sc_f = sc_b = None
    if c['train']:
        m = mask.reshape(N, R).to(f32)
        inv_keep = one / torch.tensor(c['keep'], dtype=f32)
        sc_f = (_neighbour_bit(m) if mut == 'keep_bit_fwd' else m) * inv_keep
        sc_b = (_neighbour_bit(m) if mut == 'keep_bit_bwd' else m) * inv_keep
    Fd = F if sc_f is None else F * sc_f
    nslab = (R + SLAB - 1) // SLAB
    part = torch.stack([Fd[:, s * SLAB:(s + 1) * SLAB] @ W[s * SLAB:(s + 1) * SLAB] for s in range(nslab)])
    logits = (part[:-1] if mut == 'logits_slab_left_out' else part).sum(0) + b
    dF = G @ W.t()
    Fdb = F
    if sc_b is not None:
        dF, Fdb = dF * sc_b, F * sc_b
    dW = None
    for nb in range(0, N, IMG_BLOCK):
        t = Fdb[nb:nb + IMG_BLOCK].t() @ G[nb:nb + IMG_BLOCK]
        dW = t if (dW is None or mut == 'dW_stored') else dW + t
    db = G.sum(0)
    g = dF.reshape(N, M, C) * invP
    dX = torch.einsum('npm,nmc->npc', A, g)
    if c['acc'] and mut != 'dX0_ignored':
        dX = dX + I['dX0'].float()
    dX = dX.to(TDT[c['dt']])
    npool = (C + SLAB - 1) // SLAB
    dA = torch.stack([torch.einsum('npc,nmc->npm', X[..., s * SLAB:(s + 1) * SLAB], g[..., s * SLAB:(s + 1) * SLAB])
                      for s in range(npool)])
    d = (dA[:-1] if mut == 'dA_last_slab_dropped' else dA).sum(0)
    add = torch.zeros(N, P, J, dtype=f32)
    for mi, j in enumerate(sel):
        add[..., j] += d[..., mi]
    if c['avged']:
        add += (d[..., nsel] * (one / nsel if mut == 'fold_mean_div_nsel' else invJ))[..., None]
    dPl = add if mut == 'dPl_stored' else I['dPl0'] + add
    if nsel + (1 if c['avged'] else 0) == 0 and mut != 'dPl_stored':
        dPl = I['dPl0'].clone()
    return dict(F=F, part=part, logits=logits, dF=dF, dW=dW, db=db, dX=dX, dA=dA, dPl=dPl)
