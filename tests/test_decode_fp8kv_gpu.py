"""GPU parity of decode_attention_fp8kv (csrc/attention_fp8kv.hip) against plain torch: the quantising cache write bit for bit,
the attention against float64 softmax attention over the dequantised cache as it stands after the write.  The bounds are the
ones tests/test_attention_gpu.py holds the bf16 decode kernel to: the fp8 -> bf16 conversion is exact and the arithmetic
after it is the same."""
import pytest
import torch

pytestmark = pytest.mark.gpu
FP8, BF16 = torch.float8_e4m3fn, torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    import sgl_kernel  # noqa: F401
    assert torch.cuda.is_available()
    return torch.ops.sgl_kernel


def quant(x, scale):
    return (x.float() / scale).clamp(-448, 448).to(FP8)


def setup(B, HQ, HKV, D, DV, aliased, seqs, idx=torch.int64, seed=0):
    """Host tensors of one call: a randn cache cast to e4m3, page tables that are a random permutation of its rows."""
    g = torch.Generator().manual_seed(seed)
    tokens = sum(seqs) + 5
    kb = torch.randn(tokens, HKV, D, generator=g).to(FP8)
    vb = kb[..., :DV] if aliased else torch.randn(tokens, HKV, DV, generator=g).to(FP8)
    perm = torch.randperm(tokens, generator=g)
    rtt = torch.zeros(B, max(seqs) + 3, dtype=idx)
    for b, n in enumerate(seqs):
        rtt[b, :n] = perm[sum(seqs[:b]):sum(seqs[:b]) + n]
    loc = torch.stack([rtt[b, n - 1] for b, n in enumerate(seqs)])
    t = dict(q=torch.randn(B, HQ, D, generator=g).to(BF16), kb=kb, vb=vb, key=torch.randn(B, HKV, D, generator=g).to(BF16),
             value=torch.randn(B, HKV, DV, generator=g).to(BF16), rtt=rtt, loc=loc, seq=torch.tensor(seqs), ridx=torch.arange(B))
    return t


def run(ops, t, depth, sm_scale, cap, ks, vs):
    """The call on device copies (an aliased v_buffer stays a view of k_buffer) -> output, k cache, v cache on the host."""
    d = {k: v.cuda() for k, v in t.items()}
    if t["vb"].data_ptr() == t["kb"].data_ptr():
        d["vb"] = d["kb"][..., :t["vb"].shape[2]]
    B, HQ, DV = t["q"].shape[0], t["q"].shape[1], t["vb"].shape[2]
    out = torch.full((B, HQ, DV), float("nan"), dtype=BF16, device="cuda")
    logits = torch.full((B, HQ, depth, DV + 1), float("nan"), device="cuda")
    assert ops.decode_attention_fp8kv(d["q"], d["kb"], d["vb"], out, d["key"], d["value"], d["loc"], logits, d["rtt"], d["ridx"],
                                      d["seq"], sm_scale, cap, ks, vs) is None
    return out.cpu(), d["kb"].cpu(), d["vb"].cpu()


def written(t, ks, vs):
    """The cache after the expected write (value wins in an aliased cache's first DV columns)."""
    kb = t["kb"].clone()
    vb = kb[..., :t["vb"].shape[2]] if t["vb"].data_ptr() == t["kb"].data_ptr() else t["vb"].clone()
    kb.view(torch.uint8)[t["loc"].long()] = quant(t["key"], ks).view(torch.uint8)
    vb.view(torch.uint8)[t["loc"].long()] = quant(t["value"], vs).view(torch.uint8)
    return kb, vb


def reference(t, kb, vb, sm_scale, cap, ks, vs):
    B, HQ, _ = t["q"].shape
    group = HQ // kb.shape[1]
    kb, vb = kb.double(), vb.double()
    ref = torch.zeros(B, HQ, vb.shape[2], dtype=torch.float64)
    for b in range(B):
        rows = t["rtt"][b, :int(t["seq"][b])].long()
        for h in range(HQ):
            s = sm_scale * ks * (kb[rows, h // group] @ t["q"][b, h].double())
            if cap > 0:
                s = cap * torch.tanh(s / cap)
            ref[b, h] = vs * (torch.softmax(s, 0) @ vb[rows, h // group])
    return ref


def close(got, ref):
    rel = ((got.double() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt().item()
    print(f"relative rms error {rel:.2e}, max |err| {(got.double() - ref).abs().max().item():.2e}")
    return rel < 6e-3 and torch.allclose(got.double(), ref, rtol=0, atol=3e-2)


#        B  HQ HKV   D   DV aliased  seq lens             idx          cap  (k_scale, v_scale)
CASES = [(3, 22, 1, 576, 512, True, [65, 300, 1], torch.int64, 0.0, (1.0, 1.0)),
         (4, 16, 4, 128, 128, False, [63, 64, 130, 300], torch.int32, 30.0, (0.5, 2.0)),
         (2, 8, 2, 192, 128, False, [130, 65], torch.int64, 0.0, (1.0, 1.0)),
         (3, 8, 8, 64, 64, False, [1, 300, 64], torch.int64, 0.0, (0.5, 2.0)),
         # The groups (HQ / HKV) at which launch_by_group takes another form, decode_fp8kv_kernel<D, DV, alias, CT, NDV, KH>: CT is 1
         # up to 16 heads, 2 up to 32 and on wide heads (D >= 256), else 4; wide heads above 32 take two workgroups per kv head
         (3, 24, 1, 128, 128, False, [63, 130, 300], torch.int64, 0.0, (0.5, 2.0)),    # <128, 128, false, 2, 1, 2>: CT = 2, narrow
         (3, 40, 1, 128, 128, False, [64, 65, 300], torch.int32, 0.0, (0.5, 2.0)),     # <128, 128, false, 4, 1, 1>: third tile half full
         (3, 64, 1, 128, 128, False, [1, 63, 130], torch.int64, 0.0, (0.5, 2.0)),      # <128, 128, false, 4, 1, 1>: four full tiles
         (3, 33, 1, 64, 64, False, [65, 130, 300], torch.int64, 0.0, (0.5, 2.0)),      # <64, 64, false, 4, 1, 1>: one head in the third
         (2, 24, 1, 192, 128, False, [130, 65], torch.int64, 0.0, (0.5, 2.0)),         # <192, 128, false, 2, 1, 2>
         (3, 16, 1, 576, 512, True, [65, 300, 1], torch.int64, 0.0, (1.0, 1.0)),       # <576, 512, true, 1, 4, 2>: a full column tile
         (3, 40, 1, 576, 512, True, [65, 300, 1], torch.int64, 0.0, (1.0, 1.0)),       # <576, 512, true, 2, 2, 2>, grid.y = 2: 32 + 8 heads
         (3, 64, 1, 576, 512, True, [65, 300, 1], torch.int64, 0.0, (1.0, 1.0))]       # <576, 512, true, 2, 2, 2>, grid.y = 2: 32 + 32 heads


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("B,HQ,HKV,D,DV,aliased,seqs,idx,cap,scales", CASES)
def test_parity(ops, B, HQ, HKV, D, DV, aliased, seqs, idx, cap, scales, depth):
    t = setup(B, HQ, HKV, D, DV, aliased, seqs, idx, seed=D + depth)
    sm = 1.0 / D ** 0.5
    out, kb, vb = run(ops, t, depth, sm, cap, *scales)
    kb_ref, vb_ref = written(t, *scales)
    assert torch.equal(kb.view(torch.uint8), kb_ref.view(torch.uint8)) and torch.equal(vb.view(torch.uint8), vb_ref.view(torch.uint8))
    assert close(out, reference(t, kb_ref, vb_ref, sm, cap, *scales))


@pytest.mark.parametrize("case,scales", [(0, (1.0, 1.0)), (1, (0.3, 0.5))])
def test_cache_write_bit_for_bit(ops, case, scales):
    """Saturation beyond +-448 scale, e4m3's subnormal range, exact ties (1.0625 lies between 1.0 and 1.125), a division that
    matters (0.3); rows other than loc keep their bytes."""
    B, HQ, HKV, D, DV, aliased, seqs = CASES[case][:7]
    t = setup(B, HQ, HKV, D, DV, aliased, seqs, seed=5)
    special = torch.tensor([1000.0, -1000.0, 448.0, 460.0, 0.003, -0.0011, 2.0 ** -10, 1.0625, -1.1875, 0.0, 3.25, 208.0])
    for x, s in ((t["key"], scales[0]), (t["value"], scales[1])):
        x[:, :, 8:8 + special.numel()] = (special * s).to(BF16)
        x[:, :, 40:40 + special.numel()] = special.to(BF16)
    _, kb, vb = run(ops, t, 2, 0.1, 0.0, *scales)
    kb_ref, vb_ref = written(t, *scales)
    assert not torch.equal(kb_ref.view(torch.uint8), t["kb"].view(torch.uint8))
    assert torch.equal(kb.view(torch.uint8), kb_ref.view(torch.uint8))
    assert torch.equal(vb.view(torch.uint8), vb_ref.view(torch.uint8))
    if aliased:
        assert torch.equal(kb.view(torch.uint8)[t["loc"].long()][..., :DV], quant(t["value"], scales[1]).view(torch.uint8))


@pytest.mark.parametrize("case,depth,scales", [(0, 1, (1.0, 1.0)), (1, 8, (0.5, 2.0)), (3, 8, (1.0, 0.3))])
def test_one_key_returns_the_value_row(ops, case, depth, scales):
    B, HQ, HKV, D, DV, aliased = CASES[case][:6]
    t = setup(B, HQ, HKV, D, DV, aliased, [1] * B, seed=9)
    out, _, vb = run(ops, t, depth, 0.3, 0.0, *scales)
    want = (vb.float()[t["loc"].long()] * scales[1]).to(BF16).repeat_interleave(HQ // HKV, 1)
    assert torch.equal(out, want)


def test_equal_keys_give_the_mean_of_v(ops):
    B, HQ, HKV, D, DV, aliased, seqs = CASES[1][:7]
    t = setup(B, HQ, HKV, D, DV, aliased, seqs, seed=3)
    t["kb"].view(torch.uint8)[:] = t["kb"].view(torch.uint8)[0].clone()
    t["key"][:] = t["kb"][0].to(BF16)
    out, kb, vb = run(ops, t, 8, 0.2, 0.0, 1.0, 2.0)
    ref = torch.stack([2.0 * vb.double()[t["rtt"][b, :n].long()].mean(0) for b, n in enumerate(seqs)]).repeat_interleave(HQ // HKV, 1)
    assert close(out, ref)


@pytest.mark.parametrize("why", ["bf16 buffers", "aliased cache, two scales", "stride not a multiple of 16", "head dims not built"])
def test_rejections_leave_the_buffers_alone(ops, why):
    B, HQ, HKV, D, DV, aliased, seqs = CASES[0][:7] if why.startswith("aliased") else CASES[1][:7]
    D, DV = (96, 96) if why.startswith("head") else (D, DV)
    t = setup(B, HQ, HKV, D, DV, aliased, seqs, seed=1)
    d = {k: v.cuda() for k, v in t.items()}
    scales = (1.0, 1.0)
    if why.startswith("bf16"):
        d["kb"], d["vb"] = d["kb"].to(BF16), d["vb"].to(BF16)
    elif why.startswith("aliased"):
        d["vb"], scales = d["kb"][..., :DV], (1.0, 2.0)
    elif why.startswith("stride"):
        d["kb"] = torch.zeros(d["kb"].shape[0], HKV, D + 8, device="cuda").to(FP8)[..., :D]
    out = torch.zeros(B, HQ, DV, dtype=BF16, device="cuda")
    logits = torch.zeros(B, HQ, 4, DV + 1, device="cuda")
    before = [d[k].clone() for k in ("kb", "vb")]
    with pytest.raises(RuntimeError):
        ops.decode_attention_fp8kv(d["q"], d["kb"], d["vb"], out, d["key"], d["value"], d["loc"], logits, d["rtt"], d["ridx"],
                                   d["seq"], 0.1, 0.0, *scales)
    torch.cuda.synchronize()
    for now, was in zip((d["kb"], d["vb"]), before):
        assert torch.equal(now.view(torch.uint8 if now.dtype == FP8 else now.dtype), was.view(torch.uint8 if was.dtype == FP8 else was.dtype))
    assert not bool(out.any())
