"""Cases, inputs, float64 reference, error bound and an emulation of ip_xattn_kernel's arithmetic (with one-defect
mutants of it), shared by tests/test_ip_attention_plan.py (CPU) and tests/test_ip_attention_gpu.py (GPU).  Nothing
here touches a device.

  out = softmax(q k^T / sqrt d) v + lambda softmax(q k_ip^T / sqrt d) v_ip

A case names the form sd_ip_attention_plan must report for it: "single" (as many blocks per (batch, head) as 64-query
tiles, one tile per block) or "walk" (fewer blocks than tiles, in uneven rounds, the last tile ragged); the CPU suite
checks that, the GPU suite runs the cases."""
import collections
import functools
import math
import zlib

import torch

LOG2E = 1.4426950408889634
HEAD_DIMS = (32, 40, 64, 80, 160)
TQ_EDGES = (1, 15, 16, 17, 63, 64, 65, 129)         # around the 16-query sub-tile and the 64-query block tile
L_EDGES = (1, 31, 32, 33, 77, 154, 160)             # around the 32-key step, up to the longest text
TIP_EDGES = (1, 4, 16, 31, 32, 33, 64)
LAMBDAS = (0.0, 0.01, 0.6, 1.0, -0.5, 4.0)

# group: "edge" | "walk" | "lambda" | "scores" | "constv"
# kind:  "randn" | "big_text" / "big_ip" (scores of std 60 in that segment) | "neg_text" / "neg_ip" (every score of that
#        segment about -150) | "constv" (v and v_ip constant per column)
Case = collections.namedtuple("Case", "group B heads Tq L Tip d lam presc kind form")


def case_id(c):
    return "%s-d%d-B%dxH%d-Tq%d-L%d-T%d-lam%g%s-%s-%s" % (c.group, c.d, c.B, c.heads, c.Tq, c.L, c.Tip, c.lam,
                                                        "-presc" if c.presc else "", c.kind, c.form)


def _build():
    cases = []

    def add(group, d, B, heads, Tq, L, Tip, lam, presc=0, kind="randn", form="single"):
        cases.append(Case(group, B, heads, Tq, L, Tip, d, lam, presc, kind, form))

    for i, d in enumerate(HEAD_DIMS):
        heads = 2 if d == 160 else 3
        # tile edges: eight cases per head dim, in which every Tq, L and T_ip edge occurs (the index of L and T_ip
        # runs through eight consecutive residues mod 7); B = 2 and heads >= 2 make every offset non-zero
        for j, Tq in enumerate(TQ_EDGES):
            add("edge", d, 2, heads, Tq, L_EDGES[(j + i) % 7], TIP_EDGES[(j + 2 * i) % 7], LAMBDAS[1 + (i + j) % 5],
                presc=j % 2)
        # every lambda, 0 included; Tq = 40 and T_ip = 5 leave rows and keys past the end of a tile and a step
        for j, lam in enumerate(LAMBDAS):
            add("lambda", d, 2, 2, 40, 45, 5, lam, presc=(i + j) % 2)
        # the stress inputs, each on either segment
        for j, kind in enumerate(("big_text", "big_ip", "neg_text", "neg_ip")):
            add("scores", d, 2, 2, 97, 77, 16, 0.8 if kind.startswith("neg") else 1.0, presc=(i + j) % 2, kind=kind)
        add("constv", d, 2, heads, 70, 77, 4, (0.6, -0.5, 4.0, 1.0, 0.01)[i], presc=i % 2, kind="constv")
    # the walk: B heads tiles > 1024, so a (batch, head) gets fewer blocks than tiles; rounds uneven, last tile ragged
    add("walk", 32, 8, 16, 64 * 19 + 3, 77, 4, 0.6, presc=1, form="walk")
    add("walk", 40, 4, 32, 64 * 9 + 17, 33, 16, 1.0, form="walk")
    add("walk", 64, 8, 8, 64 * 17 + 1, 154, 64, -0.5, form="walk")
    add("walk", 80, 2, 32, 64 * 20 + 63, 77, 33, 4.0, presc=1, form="walk")
    add("walk", 160, 8, 4, 64 * 33 + 17, 77, 16, 0.6, form="walk")
    return cases


GPU_CASES = _build()


def seed_of(case):
    return zlib.crc32(case_id(case).encode()) & 0x7fffffff


def make_inputs(case):
    """fp16 q [B, Tq, heads d] (carrying log2(e) / sqrt(d) when case.presc), k, v [B, L, heads d], k_ip, v_ip
    [B, T_ip, heads d]."""
    B, H, Tq, L, Tip, d = case.B, case.heads, case.Tq, case.L, case.Tip, case.d
    C = H * d
    g = torch.Generator().manual_seed(seed_of(case))
    c = LOG2E / math.sqrt(d) if case.presc else 1.0
    q = torch.randn(B, Tq, C, generator=g)
    k = torch.randn(B, L, C, generator=g)
    v = torch.randn(B, L, C, generator=g)
    kip = torch.randn(B, Tip, C, generator=g)
    vip = torch.randn(B, Tip, C, generator=g)
    if case.kind == "big_text":
        k *= 60.0
    if case.kind == "big_ip":
        kip *= 60.0
    if case.kind.startswith("neg"):
        q = torch.rand(B, Tq, C, generator=g) + 0.5
        T = L if case.kind == "neg_text" else Tip
        neg = -(torch.rand(B, T, C, generator=g) + 2.0) * (60.0 / math.sqrt(d))
        if case.kind == "neg_text":
            k = neg
        else:
            kip = neg
    if case.kind == "constv":
        a = torch.randn(C, generator=g) * 3.0
        b = torch.randn(C, generator=g) * 3.0
        a[::7] = -a[::7].abs() - 0.01
        b[3::11] *= 1e-3
        v = a.expand(B, L, C).clone()
        vip = b.expand(B, Tip, C).clone()
    return (q * c).half(), k.half(), v.half(), kip.half(), vip.half()


def _heads(t, T, H, d):
    return t.view(1, T, H, d).transpose(1, 2)


def reference(case, q, k, v, kip, vip):
    """float64 of the fp16 operands: O and A = softmax(..) |v| + |lambda| softmax(..) |v_ip|, both [B, Tq, heads d].
    Pre-scaled queries are un-scaled first."""
    B, H, Tq, L, Tip, d = case.B, case.heads, case.Tq, case.L, case.Tip, case.d
    O = torch.empty(B, Tq, H * d, dtype=torch.float64)
    A = torch.empty_like(O)
    unscale = math.sqrt(d) / LOG2E if case.presc else 1.0
    for b in range(B):
        qd = _heads(q[b].double() * unscale, Tq, H, d)
        o = torch.zeros(1, H, Tq, d, dtype=torch.float64)
        a = torch.zeros_like(o)
        for kk, vv, T, coef in ((k, v, L, 1.0), (kip, vip, Tip, case.lam)):
            vd = _heads(vv[b].double(), T, H, d)
            P = torch.softmax(qd @ _heads(kk[b].double(), T, H, d).transpose(-1, -2) / math.sqrt(d), dim=-1)
            o += coef * (P @ vd)
            a += abs(coef) * (P @ vd.abs())
        O[b] = o.transpose(1, 2).reshape(Tq, H * d)
        A[b] = a.transpose(1, 2).reshape(Tq, H * d)
    return O, A


@functools.lru_cache(maxsize=2)
def inputs_and_reference(case):
    """(q, k, v, k_ip, v_ip, O, A) of a case, computed once for the tests that run it; callers must not modify them."""
    ins = make_inputs(case)
    return ins + reference(case, *ins)


def elementwise_bound(O, A, n_keys, vmax, lam):
    """|out - O| may not exceed this; n_keys = L + T_ip, vmax = max(|v|, |v_ip|).  attn_cases.elementwise_bound restated
    for the arithmetic of ip_segment (ip_attention_blocks.h), term by term:

      * each segment's softmax is exact in form: fp32 scores, their exact maximum m, p = exp2(fma(s, c, -m c)),
        l = sum p in fp32, w = coef / l in fp32 (coef = 1 for the text, lambda for the image segment).  What this leaves
        on a normalised probability coef p / l is relative: the fp32 rounding of the score sums (ln 2 times the error
        of a log2-domain score, on p and again, partly cancelling, on l), the hardware exp2 (an ulp or two of fp32),
        the fp32 row sum, the division and the product p w (2^-24 each).  Budget 3 * 2^-11 of A, i.e. score errors
        up to about 2^-11 in the log2 domain: 16 fp32 ulps of a score of magnitude 256, the size of the stress inputs;
      * P = fp16(p w), rounded to nearest: 2^-11 relative for a normal result, 2^-11 A.  With the line above: 2^-9 A;
      * a P below 2^-14 lands in fp16's subnormal range, where rounding to nearest loses up to 2^-25 absolute,
        whatever lambda made it small; at most n_keys of them, each times |v| <= vmax:  n_keys 2^-25 vmax;
      * both segments add into one fp32 accumulator, n_keys additions; a partial sum is at most (1 + |lambda|) vmax
        <= 2 max(1, |lambda|) vmax, each addition rounds by 2^-24 of it:  n_keys 2^-23 max(1, |lambda|) vmax;
      * one fp16 store, 2^-11 |out| <= 2^-11 (|O| + the error so far); 2^-10 |O| covers that second-order part;
      * an output in the subnormal range: 2^-25, written as 2^-24 like the bound this restates."""
    return (2.0 ** -9 * A + 2.0 ** -10 * O.abs() + n_keys * (2.0 ** -23 * max(1.0, abs(lam)) + 2.0 ** -25) * vmax
            + 2.0 ** -24)


def bound_of(case, v, vip, O, A):
    vmax = max(v.abs().max().item(), vip.abs().max().item())
    return elementwise_bound(O, A, case.L + case.Tip, vmax, case.lam)


# ------------------------------------------------------------------------------------------------ emulation
MUTANTS = ("lambda_off_last_step", "last_key_masked", "key_past_end", "subtile_from_next_tile", "joint_sum",
           "lambda_after_rounding")


def _fma(a, c, b):
    """fp32 fma(a, c, b): the product of two fp32 values is exact in float64."""
    return (a.double() * float(c) + b.double()).float()


def _segment(qf, kk, vv, n, coef, c, mutant, is_ip, joint=None):
    """One segment as ip_segment runs it, on K / V zero-padded to whole 32-key steps: returns (fp32 PV contribution
    [1, H, Tq, d], row maximum, p) -- the latter two for the joint-sum mutant."""
    H, d = qf.shape[1], qf.shape[3]
    rows = 32 * ((n + 31) // 32)
    kp = torch.zeros(rows, H * d)
    vp = torch.zeros(rows, H * d)
    kp[:n] = kk.float()
    vp[:n] = vv.float()
    S = qf @ _heads(kp, rows, H, d).transpose(-1, -2)                 # fp32 scores, a padded key scores 0
    valid = n
    if mutant == "last_key_masked":
        valid = n - 1
    if mutant == "key_past_end":
        valid = min(n + 1, rows)
    S[..., valid:] = float("-inf")
    m = S.amax(dim=-1, keepdim=True)
    if joint is not None:
        m = torch.maximum(m, joint)
    p = torch.exp2(_fma(S, c, -m * c))
    return S, m, p, _heads(vp, rows, H, d), rows


def emulate(case, q, k, v, kip, vip, mutant=None):
    """The kernel's arithmetic in torch on the CPU: per segment fp32 scores in the log2 domain on K / V padded with
    zero rows to whole 32-key steps, keys >= n masked, the exact maximum, p = exp2(fma(s, c, -m c)), l = sum p in fp32,
    w = coef / l, P = fp16(p w) rounded to nearest, fp32 PV, both segments into one fp32 accumulator, fp16 output.
    lambda = 0 skips the image segment.  `mutant` plants one defect (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS
    B, H, Tq, L, Tip, d = case.B, case.heads, case.Tq, case.L, case.Tip, case.d
    c = torch.tensor(1.0 if case.presc else LOG2E, dtype=torch.float32)
    if not case.presc:
        c = c / torch.sqrt(torch.tensor(float(d), dtype=torch.float32))
    lam = torch.tensor(case.lam, dtype=torch.float32)
    out = torch.empty(B, Tq, H * d, dtype=torch.float16)
    for b in range(B):
        qf = _heads(q[b].float(), Tq, H, d)
        acc = torch.zeros(1, H, Tq, d)
        segs = [(k[b], v[b], L, torch.tensor(1.0), False)]
        if case.lam != 0.0:
            segs.append((kip[b], vip[b], Tip, lam, True))
        joint = None
        if mutant == "joint_sum" and len(segs) == 2:
            ms = [_segment(qf, kk, vv, n, coef, c, None, ip)[1] for kk, vv, n, coef, ip in segs]
            joint = torch.maximum(ms[0], ms[1])
            parts = [_segment(qf, kk, vv, n, coef, c, None, ip, joint) for kk, vv, n, coef, ip in segs]
            l_joint = parts[0][2].sum(dim=-1, keepdim=True) + parts[1][2].sum(dim=-1, keepdim=True)
        for si, (kk, vv, n, coef, is_ip) in enumerate(segs):
            S, m, p, vh, rows = _segment(qf, kk, vv, n, coef, c, mutant, is_ip, joint)
            l = l_joint if joint is not None else p.sum(dim=-1, keepdim=True)
            if mutant == "lambda_after_rounding" and is_ip:
                acc = acc + coef * ((p * (1.0 / l)).half().float() @ vh)
                continue
            w = coef / l
            if mutant == "lambda_off_last_step" and is_ip:
                w = w.expand(-1, -1, -1, rows).clone()
                w[..., rows - 32:] = 1.0 / l
            acc = acc + (p * w).half().float() @ vh
        o = acc.half().transpose(1, 2).reshape(Tq, H * d)
        if mutant == "subtile_from_next_tile" and Tq >= 64 + 32:
            o = o.clone()
            o[16:32] = o[64 + 16:64 + 32]                   # the second sub-tile of tile 0 took tile 1's query rows
        out[b] = o
    return out
