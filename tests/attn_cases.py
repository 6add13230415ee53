"""Cases, inputs, float64 reference and error bound shared by tests/test_attention_plan.py (CPU) and
tests/test_attention_gpu.py (GPU).  Nothing here touches a device.

A case names the attn_kernel<D, QT, KT, PRESC, NWV> instantiation it was written for; the CPU suite checks that
sd_attention_plan gives that answer for every case and that the cases cover INSTANTIATIONS, the GPU suite runs them."""
import collections
import functools
import math
import zlib

import torch

# Every instantiation launch_attention can reach under default settings (SD_ATTN_NWV / SD_ATTN_NWV80 unset), as
# (D, QT, KT, PRESC, NWV): the answers of attention_plan() in stablediffusion_amd/csrc/attention.hip, which is also
# what launch_attention dispatches on.  A new return value there needs a row here and GPU cases below.
INSTANTIATIONS = [
    (40, 4, 64, 1, 8),      # SD1.5 64 x 64 level, 512 queries per block
    (80, 2, 64, 0, 8),      # SD1.5 32 x 32 level, 256 queries per block
    (160, 1, 64, 0, 4),     # SD1.5 16 x 16 / 8 x 8 levels at small batch, 64 queries per block
    (32, 2, 64, 1, 4),
    (32, 2, 64, 0, 4),
    (40, 4, 64, 1, 4),
    (40, 4, 64, 0, 4),
    (64, 2, 64, 0, 4),      # SDXL, CLIP (causal)
    (80, 2, 64, 0, 4),
    (128, 2, 64, 0, 4),
    (160, 2, 64, 0, 4),
    (512, 1, 64, 0, 4),     # VAE mid block, no prefetch
]
# the instantiations that sum the softmax denominator from the un-truncated fp32 probabilities (no spare PV row for a
# column of ones); the others take it from the truncated fp16 values through the PV MFMA
EXACT_DENOMINATOR = {80, 128, 160, 512}

LOG2E = 1.4426950408889634

# kind: "randn" | "spike" | "neg" | "const1" | "constmix";  layouts: the operand layouts the GPU suite runs
#   "contig"  every operand its own dense [rows, heads * d] matrix
#   "qkv"     q, k, v column slices of one [B * T, 3C + 8] buffer (UNet / VAE / CLIP self-attention)
#   "textkv"  k, v slices at a non-zero column offset of a [B * Tk, 4C + 24] row (the UNet's text K / V)
Case = collections.namedtuple("Case", "group B heads Tq Tk d causal presc kind layouts inst")


def case_id(c):
    return "%s-d%d-B%dxH%d-%dx%d%s%s-%s" % (c.group, c.d, c.B, c.heads, c.Tq, c.Tk, "-causal" if c.causal else "",
                                             "-presc" if c.presc else "", c.kind)


def queries_per_block(inst):
    return 16 * inst[1] * inst[4]


def _cdiv(a, b):
    return (a + b - 1) // b


def _batch_for(inst, Tq):
    """(B, heads) that lands a non-causal problem of Tq queries on `inst`: the smallest batch at the eight-wave /
    long-block thresholds of attention_plan, a single small batch below them."""
    d, qt, _, _, nwv = inst
    if (d, nwv) == (40, 8):
        heads = 32
        return _cdiv(512, _cdiv(Tq, 512) * heads), heads
    if (d, nwv) == (80, 8):
        heads = 32
        return _cdiv(256, _cdiv(Tq, 256) * heads), heads
    if (d, qt) == (160, 2):
        heads = 16
        return _cdiv(256, _cdiv(Tq, 128) * heads), heads
    return 1, (1 if d == 512 else 2)


def _below(inst):
    """The instantiation the same problem takes one step below `inst`'s threshold."""
    return {(40, 4, 64, 1, 8): (40, 4, 64, 1, 4), (80, 2, 64, 0, 8): (80, 2, 64, 0, 4),
            (160, 2, 64, 0, 4): (160, 1, 64, 0, 4)}[inst]


def _build():
    cases = []

    def add(group, B, heads, Tq, Tk, d, inst, causal=0, presc=0, kind="randn", layouts=("contig",)):
        cases.append(Case(group, B, heads, Tq, Tk, d, causal, presc, kind, tuple(layouts), tuple(inst)))

    # ---- the three instantiations no operator test reached, at their thresholds and half the batch below ----
    newly = [((40, 4, 64, 1, 8), [(16, 32, 130, 130), (8, 32, 515, 77), (8, 32, 515, 515)], (1,)),
             ((80, 2, 64, 0, 8), [(8, 32, 200, 200), (8, 16, 300, 77), (8, 16, 257, 129)], (0, 1)),
             ((160, 2, 64, 0, 4), [(8, 16, 150, 150), (8, 32, 64, 64)], (0, 1))]
    for inst, shapes, prescs in newly:
        for (B, heads, Tq, Tk) in shapes:
            for presc in prescs:
                add("threshold", B, heads, Tq, Tk, inst[0], inst, presc=presc)
                add("threshold", B // 2, heads, Tq, Tk, inst[0], _below(inst), presc=presc)

    # ---- key counts at the edges of the 64-key tile, query counts at the edges of a block ----
    for inst in INSTANTIATIONS:
        qb = queries_per_block(inst)
        for Tq, Tk in [(1, 1), (qb - 1, 16), (qb, 63), (qb + 1, 64), (qb + 1, 65), (qb - 1, 128), (qb, 129)]:
            B, heads = _batch_for(inst, Tq)
            add("edge", B, heads, Tq, Tk, inst[0], inst, presc=inst[3])

    # ---- strided operands and sentinels, for the instantiations the UNet, the VAE and CLIP run ----
    p = 1      # the UNet's queries are pre-scaled
    add("strided", 16, 32, 130, 130, 40, (40, 4, 64, 1, 8), presc=p, layouts=("contig", "qkv"))
    add("strided", 8, 32, 515, 77, 40, (40, 4, 64, 1, 8), presc=p, layouts=("contig", "textkv"))
    add("strided", 8, 32, 130, 130, 40, (40, 4, 64, 1, 4), presc=p, layouts=("contig", "qkv"))
    add("strided", 2, 8, 300, 77, 40, (40, 4, 64, 1, 4), presc=p, layouts=("contig", "textkv"))
    add("strided", 8, 32, 200, 200, 80, (80, 2, 64, 0, 8), presc=p, layouts=("contig", "qkv"))
    add("strided", 8, 16, 300, 77, 80, (80, 2, 64, 0, 8), presc=p, layouts=("contig", "textkv"))
    add("strided", 4, 32, 200, 200, 80, (80, 2, 64, 0, 4), presc=p, layouts=("contig", "qkv"))
    add("strided", 2, 8, 150, 77, 80, (80, 2, 64, 0, 4), presc=p, layouts=("contig", "textkv"))
    add("strided", 8, 16, 150, 150, 160, (160, 2, 64, 0, 4), presc=p, layouts=("contig", "qkv"))
    add("strided", 8, 16, 150, 77, 160, (160, 2, 64, 0, 4), presc=p, layouts=("contig", "textkv"))
    add("strided", 2, 8, 70, 70, 160, (160, 1, 64, 0, 4), presc=p, layouts=("contig", "qkv"))
    add("strided", 2, 8, 70, 77, 160, (160, 1, 64, 0, 4), presc=p, layouts=("contig", "textkv"))
    add("strided", 2, 5, 140, 140, 64, (64, 2, 64, 0, 4), presc=p, layouts=("contig", "qkv"))          # SDXL
    add("strided", 2, 5, 140, 77, 64, (64, 2, 64, 0, 4), presc=p, layouts=("contig", "textkv"))
    add("strided", 2, 4, 140, 140, 32, (32, 2, 64, 1, 4), presc=p, layouts=("contig", "qkv"))          # tiny test UNet
    add("strided", 2, 4, 140, 77, 32, (32, 2, 64, 1, 4), presc=p, layouts=("contig", "textkv"))
    add("strided", 2, 1, 130, 130, 512, (512, 1, 64, 0, 4), layouts=("contig", "qkv"))                 # VAE
    add("strided", 2, 1, 130, 130, 128, (128, 2, 64, 0, 4), layouts=("contig", "qkv"))                 # tiny VAE

    # ---- causal, the CLIP form ----
    for T in (64, 65, 77, 128, 129):
        add("causal", 2, 3, T, T, 64, (64, 2, 64, 0, 4), causal=1, layouts=("contig", "qkv"))

    # ---- constant V: the normalisation alone ----
    smallest = {(40, 4, 64, 1, 8): (16, 32, 130, 130), (80, 2, 64, 0, 8): (8, 32, 200, 200),
                (160, 2, 64, 0, 4): (8, 16, 150, 150)}
    for inst in INSTANTIATIONS:
        B, heads, Tq, Tk = smallest.get(inst, _batch_for(inst, 150) + (150, 150))
        for kind in ("const1", "constmix"):
            add("constv", B, heads, Tq, Tk, inst[0], inst, presc=inst[3], kind=kind)

    # ---- a score spike in the last key tile, and scores far below zero, on the newly reached instantiations ----
    for inst, (B, heads, Tq, Tk), prescs in [((40, 4, 64, 1, 8), (16, 32, 130, 130), (1,)),
                                             ((80, 2, 64, 0, 8), (8, 32, 200, 200), (0, 1)),
                                             ((160, 2, 64, 0, 4), (8, 16, 150, 150), (0, 1))]:
        for presc in prescs:
            for kind in ("spike", "neg"):
                add("extreme", B, heads, Tq, Tk, inst[0], inst, presc=presc, kind=kind)
    return cases


GPU_CASES = _build()


def seed_of(case):
    return zlib.crc32(case_id(case).encode()) & 0x7fffffff


def make_inputs(case):
    """fp16 q [B, Tq, heads * d] (carrying log2(e) / sqrt(d) when case.presc), k and v [B, Tk, heads * d]."""
    B, H, Tq, Tk, d = case.B, case.heads, case.Tq, case.Tk, case.d
    C = H * d
    g = torch.Generator().manual_seed(seed_of(case))
    c = LOG2E / math.sqrt(d) if case.presc else 1.0
    if case.kind == "neg":
        # every score of a row far below zero: the first tile has to pull the running reference down
        base = torch.randn(1, 1, C, generator=g)
        q = (base * 6.0).expand(B, Tq, C).clone()
        k = -base * 6.0 + 0.1 * torch.randn(B, Tk, C, generator=g)
    else:
        q = torch.randn(B, Tq, C, generator=g)
        k = torch.randn(B, Tk, C, generator=g) * (0.3 if case.kind == "spike" else 1.0)
    v = torch.randn(B, Tk, C, generator=g)
    q = (q * c).half()
    if case.kind == "spike":
        # one key far above the rest for a query of the first wave and for the last query, both keys in the LAST tile
        assert (Tk - 2) // 64 == (Tk - 1) // 64 and Tk > 64
        k[:, Tk - 1] = q[:, min(17, Tq - 1)].float() / c * 2.0
        k[:, Tk - 2] = q[:, Tq - 1].float() / c * 2.0
    if case.kind == "const1":
        v = torch.ones(B, Tk, C)
    if case.kind == "constmix":
        row = torch.randn(C, generator=g) * 3.0
        row[::7] = -row[::7].abs() - 0.01
        row[3::11] *= 1e-3
        v = row.expand(B, Tk, C).clone()
    return q, k.half(), v.half()


def _heads(t, B, T, H, d):
    return t.view(B, T, H, d).transpose(1, 2)


def _causal_mask(Tq, Tk):
    return torch.ones(Tq, Tk, dtype=torch.bool).triu(1)


def reference(case, q, k, v):
    """float64 on the CPU of the fp16 operands: O = softmax(q k^T / sqrt(d)) v and A = softmax(..) |v|, both
    [B, Tq, heads * d] float64.  Pre-scaled queries are un-scaled first."""
    B, H, Tq, Tk, d = case.B, case.heads, case.Tq, case.Tk, case.d
    O = torch.empty(B, Tq, H * d, dtype=torch.float64)
    A = torch.empty_like(O)
    unscale = math.sqrt(d) / LOG2E if case.presc else 1.0
    for b in range(B):           # a batch item at a time keeps the score matrix small
        qd = _heads(q[b:b + 1].double() * unscale, 1, Tq, H, d)
        kd = _heads(k[b:b + 1].double(), 1, Tk, H, d)
        vd = _heads(v[b:b + 1].double(), 1, Tk, H, d)
        S = qd @ kd.transpose(-1, -2) / math.sqrt(d)
        if case.causal:
            S = S.masked_fill(_causal_mask(Tq, Tk), float("-inf"))
        P = torch.softmax(S, dim=-1)
        O[b] = (P @ vd).transpose(1, 2).reshape(Tq, H * d)
        A[b] = (P @ vd.abs()).transpose(1, 2).reshape(Tq, H * d)
    return O, A


@functools.lru_cache(maxsize=2)
def inputs_and_reference(case):
    """(q, k, v, O, A) of a case, computed once for the tests that run it; callers must not modify them."""
    q, k, v = make_inputs(case)
    return (q, k, v) + reference(case, q, k, v)


def elementwise_bound(O, A, Tk, vmax):
    """|out - O| may not exceed this.  From the kernel's stated arithmetic: probabilities truncated to fp16 (relative
    error below 2^-10) against a denominator summed from the same truncated values or from the exact ones, fp32
    accumulation over Tk keys, an fp16 store (2^-11), and probabilities in fp16's subnormal range that lose at most
    2^-24 each against a denominator of at least 1."""
    return 2.0 ** -9 * A + 2.0 ** -10 * O.abs() + Tk * 2.0 ** -23 * vmax + 2.0 ** -24


def emulate(case, q, k, v, packed_denominator):
    """The kernel's arithmetic in torch on the CPU: fp32 scores in the log2 domain, probabilities truncated to fp16
    (the low 13 mantissa bits of the fp32 value cleared, then .half()), fp32 sums, the denominator summed from the
    truncated values (packed_denominator) or from the exact ones, fp16 output."""
    B, H, Tq, Tk, d = case.B, case.heads, case.Tq, case.Tk, case.d
    out = torch.empty(B, Tq, H * d, dtype=torch.float16)
    for b in range(B):
        S = _heads(q[b:b + 1].float(), 1, Tq, H, d) @ _heads(k[b:b + 1].float(), 1, Tk, H, d).transpose(-1, -2)
        if not case.presc:
            S = S * torch.tensor(LOG2E / math.sqrt(d), dtype=torch.float32)
        if case.causal:
            S = S.masked_fill(_causal_mask(Tq, Tk), float("-inf"))
        p = torch.exp2(S - S.amax(dim=-1, keepdim=True))
        pt = (p.view(torch.int32) & -8192).view(torch.float32).half().float()
        num = pt @ _heads(v[b:b + 1].float(), 1, Tk, H, d)
        den = (pt if packed_denominator else p).sum(dim=-1, keepdim=True)
        out[b] = (num / den).half().transpose(1, 2).reshape(Tq, H * d)
    return out
