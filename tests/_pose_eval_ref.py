"""Cases, inputs and the float64 stage references of apa_pose_attn_eval_step (tests/test_pose_attn_eval_gpu.py; the
bound-size check of tests/test_pose_attn_eval_cpu.py runs the same code on the CPU).  Error model: tests/_m1_probe.py
(Bnd, contract, softmax_p, check, C_ACC, EPS32, U_BF16) with the operand rule of tests/_gemm_probe.py (a product with a
bf16 operand rounds the fp32 one to bf16).

Stage `att`.  On the fused route no pose_pre_logits map exists, so the raw attention logits Z = Ppre . wa + ba are
taken in float64 from X, the W1 operand (bf16-rounded with bf16 features), b1, wa and ba:
    per Ppre element   e_c = C_ACC (C + 8) EPS32 (|X| . |W1| + |b1|) + U_BF16 |Ppre_c|     (U_BF16 term: bf16 only)
    on Z               sum_c |wa_c| e_c + C_ACC (Cp + 8) EPS32 sum_c |wa_c Ppre_c|
relu is 1-Lipschitz: an error of the pre-activation passes through it at most undiminished, so no gate is ambiguous
and nothing is masked -- for Ppre's relu and for APA_FLAG_RELU_ATT alike.  Softmax over the pixels: _m1_probe.softmax_p.
Later stages (zsave, abar, logits) follow from the kernel's OWN att under the contraction bounds tests/test_m1_paths_gpu.py
uses; probs / loss from the kernel's own logits under that file's C_ACC (K + 16) EPS32.

Inputs: the positive-mean recipe of tests/test_pose_paths_gpu.py -- X = relu(U(-0.25, 1)) * rowscale U(0.5, 1.5), W1 =
U(-0.25, 1) / C, b1[c] = -median_r (X W1)[r, c] * U(0.9, 1.1) (about half of the gates open), W2 = U(-0.25, 1) / Cp, wa =
U(-0.25, 1) scaled so that mean |Z| is 1 (softmax: max Z = 0.75, so that 2 max|dZ| stays below 1 %); ba = U * 0.1, or
-0.5 mean Z under APA_FLAG_RELU_ATT (gates both ways, the largest outputs still of the order of the largest Z).  Image
n's channel block n (C / 8 channels) is doubled and the top-down weights of class (7 n + 3) mod K read that block with
3 / sqrt(C) more: image n's largest logit is that class, by a gap far above the logit bound (asserted)."""
import torch

from tests._m1_probe import Bnd, C_ACC, EPS32, U_BF16, contract, softmax_p

F32, BF16 = 0, 1
TDT = {F32: torch.float32, BF16: torch.bfloat16}
RELU_ATT, SOFTMAX_ATT = 2, 1


def case(name, N, P, C, Cp, J, K, *, dt=BF16, flags=0, route=1, pl=False, shadow=False, labels=False):
    return dict(name=name, N=N, P=P, C=C, Cp=Cp, J=J, K=K, dt=dt, flags=flags, route=route, pl=pl, shadow=shadow,
                labels=labels)


CASES = [
    # two column tiles; R = 675 is ragged against the row tile; image boundaries fall inside tiles
    case('fused_ragged', 3, 225, 128, 256, 16, 51),
    case('fused_relu', 2, 100, 64, 384, 16, 20, flags=RELU_ATT),
    case('fused_softmax', 2, 49, 64, 256, 16, 20, flags=SOFTMAX_ATT),
    case('fused_shadow', 4, 196, 2048, 768, 16, 393, shadow=True),
    case('composed_pl', 3, 225, 128, 256, 16, 51, route=0, pl=True),
    case('composed_cp200', 2, 43, 96, 200, 16, 10, route=0),
    case('composed_fp32', 2, 12, 64, 64, 13, 10, dt=F32, route=0, labels=True),
]


def make_inputs(c):
    """CPU tensors (the same values wherever the test runs): X in the feature dtype, everything else fp32."""
    N, P, C, Cp, J, K = c['N'], c['P'], c['C'], c['Cp'], c['J'], c['K']
    R, bf = N * P, c['dt'] == BF16
    gen = torch.Generator().manual_seed(sum(map(ord, c['name'])))
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    ro = lambda *s: rnd(*s) * 1.25 - 0.25
    X = torch.relu(ro(R, C)) * (0.5 + rnd(R, 1))
    g = C // 8
    for n in range(N):
        X[n * P:(n + 1) * P, n * g:(n + 1) * g] *= 2.0
    X = X.to(TDT[c['dt']])
    W1 = (ro(C, Cp) / C).float()
    W1v = W1.to(torch.bfloat16).double() if bf else W1.double()
    S = X.double() @ W1v
    b1 = (-S.median(dim=0).values * (0.9 + 0.2 * rnd(Cp))).float()
    W2 = (ro(Cp, J) / Cp).float()
    b2 = (torch.randn(J, generator=gen, dtype=torch.float64) * 0.1).float()
    Ppre = torch.relu(S + b1.double())
    if bf:
        Ppre = Ppre.to(torch.bfloat16).double()
    wa0 = ro(Cp)
    Z0 = Ppre @ wa0
    if c['flags'] & SOFTMAX_ATT:
        wa = (wa0 * (0.75 / float(Z0.max()))).float()
    else:
        wa = (wa0 / float(Z0.abs().mean())).float()
    Z = Ppre @ wa.double()
    relu_att = (c['flags'] & RELU_ATT) and not (c['flags'] & SOFTMAX_ATT)
    ba = (-0.5 * Z.mean().reshape(1) if relu_att else ro(1) * 0.1).float()
    Wt = ro(C, K) / C ** 0.5
    for n in range(N):
        Wt[n * g:(n + 1) * g, (7 * n + 3) % K] += 3.0 / C ** 0.5
    Wt = Wt.float()
    bt = (ro(K) * 0.1).float()
    labels = torch.randint(0, K, (N,), generator=gen)
    return dict(X=X.view(N, P, C), W1=W1, b1=b1, W2=W2, b2=b2, Wa=wa, ba=ba, Wt=Wt, bt=bt, labels=labels)


def att_reference(c, inp):
    """Bnd of the attention map as the step leaves it in `att` (id / relu: Z; softmax: over the pixels), from the
    inputs alone.  Every tensor on the device of inp['X']."""
    N, P, C, Cp = c['N'], c['P'], c['C'], c['Cp']
    bf = c['dt'] == BF16
    X = inp['X'].double().reshape(N * P, C)
    W1v = inp['W1'].to(torch.bfloat16).double() if bf else inp['W1'].double()
    b1, wa, ba = inp['b1'].double(), inp['Wa'].double().reshape(-1), inp['ba'].double()
    pre = X @ W1v + b1
    mag = X.abs() @ W1v.abs() + b1.abs()
    ppre = torch.relu(pre)
    if bf:
        ppre = ppre.to(torch.bfloat16).double()          # (the values a stored map holds: the reference of the stage)
    e_c = C_ACC * (C + 8) * EPS32 * mag + (U_BF16 * ppre.abs() if bf else 0.0)
    z = ppre @ wa + ba
    err = e_c @ wa.abs() + C_ACC * (Cp + 8) * EPS32 * (ppre * wa).abs().sum(dim=1)
    zl = Bnd(z.reshape(N, P), err.reshape(N, P))
    if c['flags'] & SOFTMAX_ATT:
        return softmax_p(zl)
    if c['flags'] & RELU_ATT:
        return Bnd(zl.ref.clamp_min(0), zl.err)
    return zl


def later_reference(c, inp, att):
    """Bnd zsave, abar, logits from the kernel's own att [N,P] (exact in float64)."""
    N, P, C, K = c['N'], c['P'], c['C'], c['K']
    A = Bnd(att.double().reshape(N, P))
    X = Bnd(inp['X'].double().reshape(N, P, C))
    zs = contract('np,npc->nc', A, X, P).scale(1.0 / P)
    ones = Bnd(torch.ones(P, dtype=torch.float64, device=att.device))
    ab = contract('np,p->n', A, ones, P).scale(1.0 / P)
    lg = contract('nc,ck->nk', zs, Bnd(inp['Wt'].double()), C) + Bnd(ab.ref[:, None], ab.err[:, None]).mul(
        Bnd(inp['bt'].double()[None, :]))
    return dict(zsave=zs, abar=ab, logits=lg.rounded())


def top_two_gap(lg):
    """(gap of the two largest reference logits per row, the largest bound of the row)"""
    top = lg.ref.topk(2, dim=1).values
    return top[:, 0] - top[:, 1], lg.err.amax(dim=1)
