"""GPU parity of extend_attention_fp8kv (csrc/attention_extend_fp8kv.hip) against plain torch: float64 softmax attention over
[float64(cache rows) * scale ; k_extend], causal on the extend part, held to the bound tests/test_attention_gpu.py holds the bf16
extend kernel to (the fp8 -> bf16 conversion is exact and the arithmetic after it is that kernel's); the optional cache write bit
for bit against the decode operator's rounding rule."""
import pytest
import torch

pytestmark = pytest.mark.gpu
FP8, BF16 = torch.float8_e4m3fn, torch.bfloat16

#        B HQ HKV HBUF  D   prefix lens     extend lens    pages        cap   (k_scale, v_scale)
CASES = [(3, 8, 2, 2, 128, [0, 65, 130], [33, 1, 300], torch.int64, 0.0, (0.3, 2.0)),   # no prefix; partial prefix tile; 2 query blocks
         (2, 4, 4, 1, 128, [64, 63], [64, 257], torch.int32, 30.0, (1.0, 1.0)),        # shared buffer head; prefix = one tile; soft cap
         (1, 4, 2, 2, 128, [450], [5], torch.int64, 0.0, (0.5, 0.25)),                 # the ring wraps twice on fp8 tiles
         (2, 4, 1, 1, 64, [1, 200], [130, 17], torch.int64, 0.0, (0.5, 0.5))]          # generic kernel


@pytest.fixture(scope="module")
def ops():
    import sgl_kernel  # noqa: F401
    assert torch.cuda.is_available()
    return torch.ops.sgl_kernel


def quant(x, scale):
    return (x.float() / scale).clamp(-448, 448).to(FP8)


def setup(case, seed=0):
    """Host tensors of one call.  The cache is filled as a server would, e4m3(clamp(randn / scale)); page tables are a random
    permutation of its rows, and `loc` names the rows the extend tokens would be written to."""
    B, HQ, HKV, HBUF, D, pre, ext, idx, cap, (ks, vs) = case
    g = torch.Generator().manual_seed(seed)
    T, tokens = sum(ext), sum(pre) + sum(ext) + 5
    perm = torch.randperm(tokens, generator=g)
    rtt = torch.zeros(B, max(p + e for p, e in zip(pre, ext)) + 3, dtype=idx)
    at = 0
    for b in range(B):
        rtt[b, :pre[b] + ext[b]] = perm[at:at + pre[b] + ext[b]]
        at += pre[b] + ext[b]
    rnd = lambda *s: torch.randn(*s, generator=g)
    return dict(q=rnd(T, HQ, D).to(BF16), k=rnd(T, HKV, D).to(BF16), v=rnd(T, HKV, D).to(BF16),
                kb=quant(rnd(tokens, HBUF, D), ks), vb=quant(rnd(tokens, HBUF, D), vs), rtt=rtt, ridx=torch.arange(B),
                seq=torch.tensor([p + e for p, e in zip(pre, ext)]), ext=torch.tensor(ext, dtype=torch.int32),
                start=torch.tensor([sum(ext[:b]) for b in range(B)], dtype=torch.int32),
                loc=torch.cat([rtt[b, pre[b]:pre[b] + ext[b]] for b in range(B)]))


def run(ops, case, t, write, d=None, scales=None):
    """The call on device copies -> output, k cache, v cache on the host."""
    d = d or {k: v.cuda() for k, v in t.items()}
    out = torch.full(t["q"].shape, float("nan"), dtype=BF16, device="cuda")
    assert ops.extend_attention_fp8kv(d["q"], d["k"], d["v"], out, d["kb"], d["vb"], d["rtt"], d["ridx"], d["seq"], d["ext"], d["start"],
                                      max(case[6]), 1.0 / case[4] ** 0.5, case[8], *(scales or case[9]),
                                      d["loc"] if write else None) is None
    return out.cpu(), d["kb"].cpu(), d["vb"].cpu()


def reference(case, t, ks, vs):
    B, HQ, HKV, HBUF, D, pre, ext, _, cap, _ = case
    ref = torch.zeros(t["q"].shape, dtype=torch.float64)
    for b in range(B):
        rows, s0, n = t["rtt"][b, :pre[b]].long(), int(t["start"][b]), ext[b]
        vis = torch.cat([torch.ones(n, pre[b]), torch.ones(n, n).tril()], 1).bool()
        for h in range(HQ):
            kv, hb = h // (HQ // HKV), (h // (HQ // HKV)) % HBUF
            K = torch.cat([t["kb"][rows, hb].double() * ks, t["k"][s0:s0 + n, kv].double()])
            V = torch.cat([t["vb"][rows, hb].double() * vs, t["v"][s0:s0 + n, kv].double()])
            s = (t["q"][s0:s0 + n, h].double() @ K.T) / D ** 0.5
            s = cap * torch.tanh(s / cap) if cap > 0 else s
            ref[s0:s0 + n, h] = torch.softmax(s.masked_fill(~vis, float("-inf")), 1) @ V
    return ref


def close(got, ref):
    print(f"max |err| {(got.double() - ref).abs().max().item():.2e}")
    return torch.allclose(got.float(), ref.bfloat16().float(), rtol=1e-2, atol=1e-2)


def same_bytes(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def written(t, ks, vs):
    kb, vb = t["kb"].clone(), t["vb"].clone()
    kb.view(torch.uint8)[t["loc"].long()] = quant(t["k"], ks).view(torch.uint8)
    vb.view(torch.uint8)[t["loc"].long()] = quant(t["v"], vs).view(torch.uint8)
    return kb, vb


@pytest.mark.parametrize("ci,write", [(c, w) for c in range(4) for w in (False, True) if not (w and CASES[c][2] != CASES[c][3])])
def test_parity(ops, ci, write):
    case = CASES[ci]
    t = setup(case, seed=ci)
    out, kb, vb = run(ops, case, t, write)
    ref = reference(case, t, *case[9])
    assert close(out, ref)
    if case[9][0] != case[9][1]:      # a missing or misplaced scale shows: the reference without the scales is out of bounds
        assert not close(ref.bfloat16(), reference(case, t, 1.0, 1.0))
    kb_ref, vb_ref = written(t, *case[9]) if write else (t["kb"], t["vb"])
    assert same_bytes(kb, kb_ref) and same_bytes(vb, vb_ref)


@pytest.mark.parametrize("ci", [0, 3])
def test_cache_write_bit_for_bit(ops, ci):
    """Saturation beyond +-448 scale, e4m3's subnormal range, exact ties (1.0625 lies between 1.0 and 1.125), a division that
    matters (0.3); rows other than out_cache_loc keep their bytes, and with None every row does."""
    case = CASES[ci]
    ks, vs = (0.3, 0.5)
    t = setup(case, seed=5)
    special = torch.tensor([1000.0, -1000.0, 448.0, 460.0, 0.003, -0.0011, 2.0 ** -10, 1.0625, -1.1875, 0.0, 3.25, 208.0])
    for x, s in ((t["k"], ks), (t["v"], vs)):
        x[:, :, 8:8 + special.numel()] = (special * s).to(BF16)
        x[:, :, 40:40 + special.numel()] = special.to(BF16)
    _, kb, vb = run(ops, case, t, True, scales=(ks, vs))
    kb_ref, vb_ref = written(t, ks, vs)
    assert not same_bytes(kb_ref, t["kb"])
    assert same_bytes(kb, kb_ref) and same_bytes(vb, vb_ref)
    _, kb, vb = run(ops, case, t, False, scales=(ks, vs))
    assert same_bytes(kb, t["kb"]) and same_bytes(vb, t["vb"])


def test_prefix_only_matches_decode_op(ops):
    """One extend token per request, its quantised rows already in the cache: extend_attention_fp8kv sees that token in bf16,
    decode_attention_fp8kv sees it quantised, so each is held to its own float64 reference on the same cache and page table."""
    B, HQ, HKV, D, lens, (ks, vs) = 3, 8, 2, 128, [65, 130, 300], (0.3, 2.0)
    case = (B, HQ, HKV, HKV, D, [n - 1 for n in lens], [1] * B, torch.int64, 0.0, (ks, vs))
    t = setup(case, seed=7)
    t["kb"], t["vb"] = written(t, ks, vs)
    out, _, _ = run(ops, case, t, False)
    assert close(out, reference(case, t, ks, vs))
    d = {k: v.cuda() for k, v in t.items()}
    dec = torch.full((B, HQ, D), float("nan"), dtype=BF16, device="cuda")
    logits = torch.empty(B, HQ, 4, D + 1, device="cuda")
    ops.decode_attention_fp8kv(d["q"], d["kb"], d["vb"], dec, d["k"], d["v"], d["loc"], logits, d["rtt"], d["ridx"], d["seq"],
                               1.0 / D ** 0.5, 0.0, ks, vs)
    ref = torch.zeros(B, HQ, D, dtype=torch.float64)      # every key from the cache, one query each
    for b in range(B):
        rows = t["rtt"][b, :lens[b]].long()
        for h in range(HQ):
            s = (t["kb"][rows, h // (HQ // HKV)].double() * ks) @ t["q"][b, h].double() / D ** 0.5
            ref[b, h] = torch.softmax(s, 0) @ (t["vb"][rows, h // (HQ // HKV)].double() * vs)
    assert close(dec.cpu(), ref)


@pytest.mark.parametrize("why", ["bf16 buffers", "stride not a multiple of 16", "head dims 192/128", "k_scale = 0",
                                 "cache write with HBUF == 1 != HKV", "out_cache_loc of the wrong length"])
def test_rejections_leave_the_buffers_alone(ops, why):
    case = CASES[1] if why.startswith("cache write") else CASES[0]
    t = setup(case, seed=1)
    d = {k: v.cuda() for k, v in t.items()}
    scales, write = case[9], why.startswith(("cache write", "out_cache_loc"))
    if why.startswith("bf16"):
        d["kb"], d["vb"] = d["kb"].to(BF16), d["vb"].to(BF16)
    elif why.startswith("stride"):
        d["kb"] = torch.zeros(d["kb"].shape[0], case[3], case[4] + 8, device="cuda").to(FP8)[..., :case[4]]
    elif why.startswith("head"):
        d["q"], d["k"] = [torch.zeros(*x.shape[:2], 192, dtype=BF16, device="cuda") for x in (d["q"], d["k"])]
        d["kb"] = torch.zeros(*d["kb"].shape[:2], 192, device="cuda").to(FP8)
    elif why.startswith("k_scale"):
        scales = (0.0, 1.0)
    elif why.startswith("out_cache_loc"):
        d["loc"] = d["loc"][:-1]
    before = [d[k].clone() for k in ("kb", "vb")]
    out = torch.zeros(t["q"].shape, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.extend_attention_fp8kv(d["q"], d["k"], d["v"], out, d["kb"], d["vb"], d["rtt"], d["ridx"], d["seq"], d["ext"], d["start"],
                                   max(case[6]), 0.1, 0.0, *scales, d["loc"] if write else None)
    torch.cuda.synchronize()
    for now, was in zip((d["kb"], d["vb"]), before):
        assert torch.equal(now.view(torch.uint8) if now.dtype == FP8 else now, was.view(torch.uint8) if was.dtype == FP8 else was)
    assert not bool(out.any())
