"""Cases, inputs, float64 reference, error bound and an emulation of region_xattn_kernel's arithmetic, shared by
tests/test_region_plan.py (CPU) and tests/test_region_attention_gpu.py (GPU).  Nothing here touches a device.

  out[n, t] = sum_r w[n % Bw, t, r] softmax(q[n, t] k[n, rL:(r+1)L]^T / sqrt(d)) v[n, rL:(r+1)L]

A case names the form sd_region_plan must pick for it ("resident": all R segments in LDS at once; "grouped": the
block restages K / V between groups of segments); the CPU suite checks that and that both forms are covered for every
head dim, the GPU suite runs the cases."""
import collections
import functools
import math
import zlib

import torch

from attn_cases import LOG2E, elementwise_bound  # noqa: F401  (the bound is attn_cases', re-exported)

HEAD_DIMS = (32, 40, 64, 80, 160)
LDS_LIMIT = 160 * 1024

# weights: "disjoint" (one-hot, region boundaries inside a 16-query tile: the first at token 23), "soft" (positive,
#          overlapping everywhere), "zero" (soft with region 1 zero everywhere), "ones" (R = 1)
# kind:    "randn" | "big" (scores of std 60 in segment R - 1) | "neg" (every score of segment 0 about -150)
Case = collections.namedtuple("Case", "B heads Tq L R d Bw presc weights kind form")


def case_id(c):
    return "d%d-R%d-L%d-B%dxH%d-Tq%d-Bw%d%s-%s-%s-%s" % (c.d, c.R, c.L, c.B, c.heads, c.Tq, c.Bw, "-presc" if c.presc else "",
                                                         c.weights, c.kind, c.form)


def _build():
    cases = []

    def add(d, R, L, Tq, weights, form, heads=2, Bw=2, presc=0, kind="randn", B=2):
        cases.append(Case(B, heads, Tq, L, R, d, Bw, presc, weights if R > 1 else "ones", kind, form))

    for d in HEAD_DIMS:
        heads = 2 if d == 160 else 3
        g3 = "grouped" if d == 160 else "resident"          # at d = 160 two 77-key segments fill the LDS
        add(d, 1, 77, 100, "ones", "resident", heads=heads)
        add(d, 2, 77, 257, "disjoint", "resident", heads=heads, presc=1)
        add(d, 3, 77, 100, "disjoint", g3, heads=heads)
        add(d, 3, 77, 64, "soft", g3, heads=heads, Bw=1)
        add(d, 3, 5, 100, "zero", "resident", heads=heads, presc=1)
        add(d, 5, 5, 257, "soft", "resident", heads=heads)
        add(d, 3, 77, 100, "soft", g3, heads=heads, kind="big")
        add(d, 3, 77, 100, "disjoint", g3, heads=heads, kind="neg", presc=1)
    # the grouped form at every head dim (the smallest R, L at which sd_region_plan has to split), disjoint and soft
    for d, R, L in [(32, 6, 160), (40, 7, 77), (64, 6, 77), (80, 5, 77), (160, 5, 77), (160, 3, 77)]:
        add(d, R, L, 100, "disjoint", "grouped", presc=1)
        add(d, R, L, 257, "zero", "grouped", Bw=1)
    add(160, 5, 77, 64, "soft", "grouped")
    add(80, 5, 5, 100, "disjoint", "resident")
    return cases


GPU_CASES = _build()


def seed_of(case):
    return zlib.crc32(case_id(case).encode()) & 0x7fffffff


def disjoint_regions(Tq, R):
    """Region index per token: the first boundary at token 23 (inside the second 16-query tile), the others 5 tokens
    past an even split of the rest."""
    cuts = [0, 23] + [23 + ((Tq - 23) * (j - 1)) // (R - 1) + 5 for j in range(2, R)] + [Tq]
    idx = torch.empty(Tq, dtype=torch.long)
    for r in range(R):
        idx[cuts[r]:cuts[r + 1]] = r
    return idx


def make_weights(case, g):
    """[Bw, Tq, R] float32, sum 1 over R for every query."""
    Bw, Tq, R = case.Bw, case.Tq, case.R
    if case.weights == "ones":
        return torch.ones(Bw, Tq, R)
    if case.weights == "disjoint":
        idx = disjoint_regions(Tq, R)
        w = torch.zeros(Bw, Tq, R)
        for b in range(Bw):
            w[b].scatter_(1, ((idx + b) % R)[:, None], 1.0)      # (another assignment per weight row)
        return w
    w = torch.rand(Bw, Tq, R, generator=g) + 0.05
    if case.weights == "zero":
        w[..., 1] = 0.0
    return w / w.sum(-1, keepdim=True)


def make_inputs(case):
    """fp16 q [B, Tq, heads d] (carrying log2(e) / sqrt(d) when case.presc), k and v [B, R L, heads d], fp32 w."""
    B, H, Tq, L, R, d = case.B, case.heads, case.Tq, case.L, case.R, case.d
    C = H * d
    g = torch.Generator().manual_seed(seed_of(case))
    c = LOG2E / math.sqrt(d) if case.presc else 1.0
    q = torch.randn(B, Tq, C, generator=g)
    k = torch.randn(B, R * L, C, generator=g)
    v = torch.randn(B, R * L, C, generator=g)
    if case.kind == "big":
        k[:, (R - 1) * L:] *= 60.0
    if case.kind == "neg":
        q = torch.rand(B, Tq, C, generator=g) + 0.5
        k[:, :L] = -(torch.rand(B, L, C, generator=g) + 2.0) * (60.0 / math.sqrt(d))
    w = make_weights(case, g)
    return (q * c).half(), k.half(), v.half(), w.float()


def _heads(t, T, H, d):
    return t.view(1, T, H, d).transpose(1, 2)


def reference(case, q, k, v, w):
    """float64 of the fp16 operands: O and A = sum_r w_r softmax_r |v_r|, both [B, Tq, heads d]."""
    B, H, Tq, L, R, d = case.B, case.heads, case.Tq, case.L, case.R, case.d
    O = torch.zeros(B, Tq, H * d, dtype=torch.float64)
    A = torch.zeros_like(O)
    unscale = math.sqrt(d) / LOG2E if case.presc else 1.0
    for b in range(B):
        qd = _heads(q[b].double() * unscale, Tq, H, d)
        for r in range(R):
            kd = _heads(k[b, r * L:(r + 1) * L].double(), L, H, d)
            vd = _heads(v[b, r * L:(r + 1) * L].double(), L, H, d)
            P = torch.softmax(qd @ kd.transpose(-1, -2) / math.sqrt(d), dim=-1)
            wr = w[b % case.Bw, :, r].double()[:, None]
            O[b] += wr * (P @ vd).transpose(1, 2).reshape(Tq, H * d)
            A[b] += wr * (P @ vd.abs()).transpose(1, 2).reshape(Tq, H * d)
    return O, A


@functools.lru_cache(maxsize=4)
def inputs_and_reference(case):
    """(q, k, v, w, O, A) of a case, computed once for the tests that run it; callers must not modify them."""
    q, k, v, w = make_inputs(case)
    return (q, k, v, w) + reference(case, q, k, v, w)


def emulate(case, q, k, v, w):
    """The kernel's arithmetic in torch on the CPU: per segment fp32 scores in the log2 domain, the exact maximum,
    p = exp2(s - max), l = sum p in fp32, P = fp16(p * (w / l)) rounded to nearest, one fp32 accumulator over all
    segments, fp16 output."""
    B, H, Tq, L, R, d = case.B, case.heads, case.Tq, case.L, case.R, case.d
    out = torch.empty(B, Tq, H * d, dtype=torch.float16)
    for b in range(B):
        qf = _heads(q[b].float(), Tq, H, d)
        acc = torch.zeros(1, H, Tq, d)
        for r in range(R):
            S = qf @ _heads(k[b, r * L:(r + 1) * L].float(), L, H, d).transpose(-1, -2)
            if not case.presc:
                S = S * torch.tensor(LOG2E / math.sqrt(d), dtype=torch.float32)
            p = torch.exp2(S - S.amax(dim=-1, keepdim=True))
            coef = w[b % case.Bw, :, r].float()[None, None, :, None] / p.sum(dim=-1, keepdim=True)
            acc = acc + (p * coef).half().float() @ _heads(v[b, r * L:(r + 1) * L].float(), L, H, d)
        out[b] = acc.half().transpose(1, 2).reshape(Tq, H * d)
    return out
