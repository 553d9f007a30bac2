"""GPU parity of decode_attention_multi (csrc/attention_decode_multi.hip) against plain torch: the cache write bit for bit, the
attention of every (request, token, head) against float64 softmax attention over the cache as it stands after the write.  The
bounds are the ones tests/test_attention_dispatch_gpu.py and tests/test_decode_fp8kv_gpu.py hold one-token decode to."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    import sgl_kernel  # noqa: F401
    assert torch.cuda.is_available()
    return torch.ops.sgl_kernel


def setup(Q, HQ, HKV, D, DV, aliased, seqs, idx=torch.int64, seed=0):
    """Host tensors of one call: a randn cache, page tables that are a random permutation of its rows.  Token t of request b sits
    at position seqs[b] - Q + t and is written to the row its page table names there (a spare row when the position is < 0)."""
    g = torch.Generator().manual_seed(seed)
    B, tokens = len(seqs), sum(seqs) + 5 + Q * len(seqs)
    kb = torch.randn(tokens, HKV, D, generator=g).to(BF16)
    vb = kb[..., :DV] if aliased else torch.randn(tokens, HKV, DV, generator=g).to(BF16)
    perm = torch.randperm(tokens, generator=g)
    rtt = torch.zeros(B, max(seqs) + 3, dtype=idx)
    for b, n in enumerate(seqs):
        rtt[b, :n] = perm[sum(seqs[:b]):sum(seqs[:b]) + n]
    spare = iter(perm[sum(seqs):].tolist())
    loc = torch.tensor([int(rtt[b, n - Q + t]) if n - Q + t >= 0 else next(spare) for b, n in enumerate(seqs) for t in range(Q)],
                       dtype=idx)
    return dict(q=torch.randn(B * Q, HQ, D, generator=g).to(BF16), kb=kb, vb=vb, key=torch.randn(B * Q, HKV, D, generator=g).to(BF16),
                value=torch.randn(B * Q, HKV, DV, generator=g).to(BF16), rtt=rtt, loc=loc, seq=torch.tensor(seqs), ridx=torch.arange(B))


def device(t):
    d = {k: v.cuda() for k, v in t.items()}
    if t["vb"].data_ptr() == t["kb"].data_ptr():           # an aliased v_buffer stays a view of k_buffer
        d["vb"] = d["kb"][..., :t["vb"].shape[2]]
    return d


def run(ops, t, Q, depth, sm_scale, cap, op="decode_attention_multi"):
    """The call on device copies, into NaN-filled output and scratch -> output, k cache, v cache on the host."""
    d = device(t)
    T, HQ, DV = t["q"].shape[0], t["q"].shape[1], t["vb"].shape[2]
    out = torch.full((T, HQ, DV), float("nan"), dtype=BF16, device="cuda")
    logits = torch.full((T, HQ, depth, DV + 1), float("nan"), device="cuda")
    head = (d["q"], d["kb"], d["vb"], out, d["key"], d["value"], d["loc"], logits, d["rtt"], d["ridx"], d["seq"])
    assert getattr(ops, op)(*head, *((Q,) if op == "decode_attention_multi" else ()), sm_scale, cap) is None
    return out.cpu(), d["kb"].cpu(), d["vb"].cpu()


def written(t):
    """The cache after the expected write (value wins in an aliased cache's first DV columns)."""
    kb = t["kb"].clone()
    vb = kb[..., :t["vb"].shape[2]] if t["vb"].data_ptr() == t["kb"].data_ptr() else t["vb"].clone()
    kb[t["loc"].long()] = t["key"]
    vb[t["loc"].long()] = t["value"]
    return kb, vb


def reference(t, Q, kb, vb, sm_scale, cap):
    T, HQ, _ = t["q"].shape
    group = HQ // kb.shape[1]
    kb, vb = kb.double().repeat_interleave(group, 1), vb.double().repeat_interleave(group, 1)
    ref = torch.zeros(T, HQ, vb.shape[2], dtype=torch.float64)
    for r in range(T):
        b, p = r // Q, int(t["seq"][r // Q]) - Q + r % Q
        if p < 0:
            continue                                        # the token sees nothing: zeros
        rows = t["rtt"][b, :p + 1].long()
        s = sm_scale * torch.einsum("khd,hd->kh", kb[rows], t["q"][r].double())
        if cap > 0:
            s = cap * torch.tanh(s / cap)
        ref[r] = torch.einsum("kh,khd->hd", torch.softmax(s, 0), vb[rows])
    return ref


def close(got, ref):
    rel = ((got.double() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt().item()
    print(f"relative rms error {rel:.2e}, max |err| {(got.double() - ref).abs().max().item():.2e}")
    return rel < 6e-3 and torch.allclose(got.double(), ref, rtol=0, atol=3e-2)


def lens(Q):
    """prefix 0 (token t sees t + 1 keys); Q = 4 drafts straddle the 64-key tile edge; two tiles and a bit; five tiles"""
    return [Q, 66, 130, 300]


#        Q  HQ HKV   D   DV aliased  cap   idx          seq lens (None = lens(Q))
CASES = [(4, 16, 4, 128, 128, False, 0.0, torch.int64, None),      # exactly one column tile
         (3, 16, 2, 128, 128, False, 30.0, torch.int32, None),     # 24 columns: tokens straddle a tile
         (5, 16, 1, 64, 64, False, 0.0, torch.int64, None),        # 80 columns: two column blocks, the second has 16
         (2, 22, 1, 576, 512, True, 0.0, torch.int32, None),       # 44 columns: on a wide head two blocks, 32 + 12
         (2, 8, 2, 192, 128, False, 0.0, torch.int64, None),
         (1, 128, 1, 576, 512, True, 0.0, torch.int64, None),      # 128 heads: the shape decode_attention_cpu rejects
         (2, 4, 1, 576, 512, False, 0.0, torch.int32, [2, 130]),   # unaliased wide cache: the single-buffered kernel form
         (4, 16, 4, 128, 128, False, 0.0, torch.int64, [2, 1])]    # fewer keys than new tokens: positions < 0 give zeros


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("Q,HQ,HKV,D,DV,aliased,cap,idx,seqs", CASES)
def test_parity(ops, Q, HQ, HKV, D, DV, aliased, cap, idx, seqs, depth):
    t = setup(Q, HQ, HKV, D, DV, aliased, seqs or lens(Q), idx, seed=D + depth)
    sm = 1.0 / D ** 0.5
    out, kb, vb = run(ops, t, Q, depth, sm, cap)
    kb_ref, vb_ref = written(t)
    assert torch.equal(kb.view(torch.int16), kb_ref.view(torch.int16)) and torch.equal(vb.view(torch.int16), vb_ref.view(torch.int16))
    assert close(out, reference(t, Q, kb_ref, vb_ref, sm, cap))


@pytest.mark.parametrize("case", [3, 5])
def test_wide_heads_on_64_column_blocks(ops, knob, case):
    """Wide heads take blocks of 32 columns by default (the cases above: 32 + 12 and 4 x 32); SGLK_DECM_WIDE_COLS=64 runs the
    44 and 128 columns as one and two blocks of 64."""
    knob(SGLK_DECM_WIDE_COLS=64)
    test_parity(ops, *CASES[case], depth=8)


def test_one_token_agrees_with_decode(ops):
    t = setup(1, 16, 4, 128, 128, False, lens(1), seed=7)
    got, kb, vb = run(ops, t, 1, 8, 0.09, 0.0)
    want, kb1, vb1 = run(ops, t, 1, 8, 0.09, 0.0, op="decode_attention_cpu")
    assert torch.equal(kb.view(torch.int16), kb1.view(torch.int16)) and torch.equal(vb.view(torch.int16), vb1.view(torch.int16))
    assert close(got, want.double())


@pytest.mark.parametrize("why", ["rows not a multiple of q_len", "q_len = 0", "head dims not built", "scratch 65 deep"])
def test_rejections_leave_the_buffers_alone(ops, why):
    D = 96 if why.startswith("head") else 128
    d = device(setup(4, 16, 4, D, D, False, lens(4), seed=1))
    q_len = {"rows": 3, "q_len": 0}.get(why.split()[0], 4)
    out = torch.zeros(16, 16, D, dtype=BF16, device="cuda")
    logits = torch.zeros(16, 16, 65 if why.startswith("scratch") else 4, D + 1, device="cuda")
    before = [d[k].clone() for k in ("kb", "vb")]
    with pytest.raises(RuntimeError):
        ops.decode_attention_multi(d["q"], d["kb"], d["vb"], out, d["key"], d["value"], d["loc"], logits, d["rtt"], d["ridx"],
                                   d["seq"], q_len, 0.1, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(d["kb"].view(torch.int16), before[0].view(torch.int16))
    assert torch.equal(d["vb"].view(torch.int16), before[1].view(torch.int16))
    assert not bool(out.any())
