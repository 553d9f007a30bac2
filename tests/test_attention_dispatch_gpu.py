"""Every kernel form the attention dispatchers can reach (csrc/attention.hip: sglk_extend_attention, sglk_flash_attn_varlen,
sglk_decode_attention), each against plain float64 softmax attention written here.  tests/test_attention_gpu.py and
tests/test_varlen_gpu.py check a handful of shapes against goldens; the dispatchers pick among many more template
instantiations and A/B knobs than those shapes reach, and a wrong constant in one of them (a column-tile to head mapping, a
per-ND register slice, a query-block size) would pass there.  The instantiation a case reaches is stated next to it, read from
the dispatch code.  (The fp8-cache decode groups are in tests/test_decode_fp8kv_gpu.py.)

Bounds are the project's own: extend / varlen allclose(ref.bfloat16(), out, rtol=1e-2, atol=1e-2) and relative RMS < 5e-3
(test_attention_gpu.py, test_varlen_gpu.py); decode relative RMS < 6e-3, allclose(atol=3e-2), cache bytes bit for bit.
Outputs start as NaN, so an unwritten row fails.  test_mutated_references_fail (CPU) shows that these predicates, at these
lengths, reject an off-by-one mask, a dropped or doubled key, swapped heads and a missing soft-cap."""
import functools

import pytest
import torch

gpu = pytest.mark.gpu
BF16 = torch.bfloat16
KEYS = 64           # keys per tile in every attention kernel (attention_internal.h: kKeys)
DEPTH = 8           # decode scratch depth (KV splits) unless a case says otherwise


@pytest.fixture(scope="module")
def ops():
    import sgl_kernel  # noqa: F401
    assert torch.cuda.is_available()
    return torch.ops.sgl_kernel


def randn(g, *shape, mul=1.0):
    return (torch.randn(*shape, generator=g) * mul).to(BF16)


# ---- float64 reference -----------------------------------------------------------------------------------------------------
def attend(q, k, v, scale, mult, cap=0.0):
    """q [HQ, Lq, D], k [HKV, Lk, D], v [HKV, Lk, DV] -> float64 [HQ, Lq, DV].  mult [Lq, Lk]: how often query i counts key j
    (0 = masked, 1 = visible; the mutants of the sensitivity test also use 2).  A query with no key gives zeros."""
    rep = q.shape[0] // k.shape[0]
    k, v = k.double().repeat_interleave(rep, 0), v.double().repeat_interleave(rep, 0)
    s = torch.einsum("hqd,hkd->hqk", q.double(), k) * scale
    if cap > 0:
        s = cap * torch.tanh(s / cap)
    w = mult.double().unsqueeze(0)
    s = s.masked_fill(w == 0, float("-inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True)) * w
    return torch.einsum("hqk,hkd->hqd", torch.nan_to_num(e / e.sum(-1, keepdim=True)), v)


def causal(P, Lq, Lk, shift=0):
    """Query i of the extend part sees keys 0 .. P + i: the mask aligned to the prefix (varlen: P = 0)."""
    return (torch.arange(Lk).view(1, Lk) <= (P + shift + torch.arange(Lq)).view(Lq, 1)).long()


def everything(P, Lq, Lk):
    return torch.ones(Lq, Lk, dtype=torch.long)


def rel_rms(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


def extend_ok(ref, out):
    """The predicate of test_attention_gpu.py::test_extend_attention and test_varlen_gpu.py::test_flash_attn_varlen."""
    return bool(torch.allclose(ref.bfloat16(), out, rtol=1e-2, atol=1e-2)) and rel_rms(out, ref) < 5e-3


def decode_ok(ref, out):
    """The predicate of test_attention_gpu.py::test_decode_attention_ragged_lengths_and_int32_index."""
    return bool(torch.allclose(out.double(), ref, atol=3e-2)) and rel_rms(out, ref) < 6e-3


def report(what, ref, out):
    print(f"{what}: relative rms error {rel_rms(out, ref):.2e}, max |err| {(out.double() - ref).abs().max().item():.2e}")


# ---- extend_attention_cpu --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extend_case(D, DV, HQ, HKV, HBUF, prefixes, extends, qmul=1.0, cap=0.0, seed=0):
    """Host tensors of one call and their reference.  The prefix lives in the cache behind a page table that is a random
    permutation (requests in reverse order of their page-table rows); the extend tokens come from k_extend / v_extend, and the
    cache rows their pages name hold other numbers, so a kernel that read those instead would be far off."""
    g = torch.Generator().manual_seed(1000 + seed)
    B, n_ext = len(prefixes), sum(extends)
    seq = [p + e for p, e in zip(prefixes, extends)]
    rows = sum(seq) + 7
    perm = torch.randperm(rows, generator=g)
    rtt = torch.zeros(B + 1, max(seq) + 2, dtype=torch.int32)
    req = torch.tensor([B - b for b in range(B)])
    at = 0
    for b, n in enumerate(seq):
        rtt[req[b], :n] = perm[at:at + n]
        at += n
    start = torch.tensor([sum(extends[:b]) for b in range(B)], dtype=torch.int32)
    c = dict(D=D, DV=DV, HQ=HQ, HKV=HKV, HBUF=HBUF, prefix=prefixes, extend=extends, cap=cap, scale=1.0 / D ** 0.5,
             q=randn(g, n_ext, HQ, D, mul=qmul), k_extend=randn(g, n_ext, HKV, D), v_extend=randn(g, n_ext, HKV, DV),
             k_buffer=randn(g, rows, HBUF, D), v_buffer=randn(g, rows, HBUF, DV), rtt=rtt, req=req,
             seq=torch.tensor(seq), ext=torch.tensor(extends, dtype=torch.int32), start=start)
    c["ref"] = extend_reference(c)
    return c


def extend_reference(c, mask=causal, cap=None, columns=None):
    """columns(P, E) -> {key position: multiplicity} edits the mask (sensitivity test)."""
    out = []
    heads = torch.arange(c["HKV"]) if c["HBUF"] == c["HKV"] else torch.zeros(c["HKV"], dtype=torch.long)
    for b, (P, E) in enumerate(zip(c["prefix"], c["extend"])):
        s = int(c["start"][b])
        toks = c["rtt"][c["req"][b], :P].long()
        k = torch.cat([c["k_buffer"][toks][:, heads], c["k_extend"][s:s + E]]).movedim(0, 1)
        v = torch.cat([c["v_buffer"][toks][:, heads], c["v_extend"][s:s + E]]).movedim(0, 1)
        mult = mask(P, E, P + E)
        for j, n in (columns(P, E) if columns else {}).items():
            if 0 <= j < P + E:
                mult[:, j] *= n
        o = attend(c["q"][s:s + E].movedim(0, 1), k, v, c["scale"], mult, c["cap"] if cap is None else cap)
        out.append(o.movedim(0, 1))
    return torch.cat(out)


def run_extend(ops, c):
    d = {k: v.cuda() for k, v in c.items() if isinstance(v, torch.Tensor) and k != "ref"}
    o = torch.full((c["q"].shape[0], c["HQ"], c["DV"]), float("nan"), dtype=BF16, device="cuda")
    assert ops.extend_attention_cpu(d["q"], d["k_extend"], d["v_extend"], o, d["k_buffer"], d["v_buffer"], d["rtt"], d["req"],
                                    d["seq"], d["ext"], d["start"], max(c["extend"]), c["scale"], c["cap"]) is None
    return o.cpu()


ALIGNED = ((0, 63, 64), (257, 1, 128))       # prefixes on both sides of a tile edge; one row past a 256-row query block
ORDERED = ((70, 0, 129), (520, 10, 300))     # 3 query blocks x 3 requests x 32 heads = 288 workgroups > 256 CUs
#             knobs                D   DV  HQ HKV HBUF  (prefixes, extends)     q*   cap
EXTEND = {
    # EXT_CASE(64, 64): extend_attention_kernel<64, 64, QT 2, FORM 0, NW 8>; one 256-row query block, then two
    "64x64": ({}, 64, 64, 4, 1, 1, ((1, 200), (130, 17)), 1.0, 0.0),
    "64x64_two_query_blocks": ({}, 64, 64, 4, 1, 1, ((130,), (300,)), 1.0, 0.0),
    # SGLK_ATTN_PP=0: the one-phase kernel where the two-phase one is the default: EXT_CASE(128, 128) <128, 128, 2, 0, 8> and
    # EXT_CASE(192, 128) <192, 128, QT 1, 0, 8> (128-row query blocks)
    "pp0_128x128": ({"SGLK_ATTN_PP": 0}, 128, 128, 4, 2, 2, ALIGNED, 1.0, 0.0),
    "pp0_192x128": ({"SGLK_ATTN_PP": 0}, 192, 128, 4, 2, 2, ALIGNED, 1.0, 0.0),
    # SGLK_ATTN_NW=4: four-wave workgroups, 128-row query blocks: <128, 96, 2, 0, 4> and <128, 128, 2, 0, 4> (never two-phase)
    "nw4_128x96": ({"SGLK_ATTN_NW": 4}, 128, 96, 4, 2, 2, ALIGNED, 1.0, 0.0),
    "nw4_128x128": ({"SGLK_ATTN_NW": 4}, 128, 128, 4, 2, 2, ALIGNED, 1.0, 0.0),
    # SGLK_ATTN_PAIR on <128, 96, 2, 0, 8> with three query blocks: paired, the middle one meets itself (part 1 breaks off)
    "pair0_three_blocks": ({"SGLK_ATTN_PAIR": 0}, 128, 96, 2, 1, 1, ((130,), (600,)), 1.0, 0.0),
    "pair1_three_blocks": ({"SGLK_ATTN_PAIR": 1}, 128, 96, 2, 1, 1, ((130,), (600,)), 1.0, 0.0),
    # SGLK_ATTN_ORDER on <128, 96, 2, 0, 8>, un-paired, more workgroups than CUs: 0 = query blocks fastest, 1 = the same with
    # the second CU-count's worth reversed, 3 = heads fastest and reversed (the default is 2)
    "order0": ({"SGLK_ATTN_ORDER": 0, "SGLK_ATTN_PAIR": 0}, 128, 96, 32, 4, 4, ORDERED, 1.0, 0.0),
    "order1": ({"SGLK_ATTN_ORDER": 1, "SGLK_ATTN_PAIR": 0}, 128, 96, 32, 4, 4, ORDERED, 1.0, 0.0),
    "order3": ({"SGLK_ATTN_ORDER": 3, "SGLK_ATTN_PAIR": 0}, 128, 96, 32, 4, 4, ORDERED, 1.0, 0.0),
    # the soft-cap in CorePP::softmax: extend_pp_kernel<0, 128> and extend_pp_kernel<0, 192>
    "cap_pp_128x128": ({}, 128, 128, 4, 2, 2, ALIGNED, 4.0, 5.0),
    "cap_pp_192x128": ({}, 192, 128, 4, 2, 2, ALIGNED, 4.0, 5.0),
    # one buffer head shared by two kv heads (kvh_buf = 0) in extend_pp_kernel<0, 128>'s HalfDma
    "pp_shared_buffer_head": ({}, 128, 128, 4, 2, 1, ((63, 130), (257, 40)), 1.0, 0.0),
}


def extend_args(name):
    knobs, D, DV, HQ, HKV, HBUF, (prefixes, extends), qmul, cap = EXTEND[name]
    # the cases that differ only in their knobs share their inputs and their reference
    return knobs, extend_case(D, DV, HQ, HKV, HBUF, prefixes, extends, qmul, cap, seed=D + DV + HQ)


@gpu
@pytest.mark.parametrize("name", list(EXTEND))
def test_extend_attention_forms(ops, knob, name):
    knobs, c = extend_args(name)
    knob(**knobs)
    out = run_extend(ops, c)
    report(name, c["ref"], out)
    assert extend_ok(c["ref"], out), name


# ---- flash_attn_varlen_func ------------------------------------------------------------------------------------------------
QLENS, KLENS = (37, 0, 300, 1), (64, 5, 300, 1)      # an empty request; two query blocks; fewer queries than keys


@functools.lru_cache(maxsize=None)
def varlen_case(D, DV, v_offset=0):
    """v_offset: v is a view that starts that many elements into rows 8 elements wider (rows then are only 4-byte aligned)."""
    g = torch.Generator().manual_seed(2000 + D + DV + v_offset)
    HQ, HKV = 4, 2
    wide = randn(g, sum(KLENS), HKV, DV + (8 if v_offset else 0))
    cu = lambda lens: torch.tensor([sum(lens[:b]) for b in range(len(lens) + 1)], dtype=torch.int32)
    return dict(q=randn(g, sum(QLENS), HQ, D), k=randn(g, sum(KLENS), HKV, D), v_wide=wide, v_offset=v_offset, DV=DV,
                cu_q=cu(QLENS), cu_k=cu(KLENS))


def varlen_v(c, wide):
    return wide[:, :, c["v_offset"]:c["v_offset"] + c["DV"]]


def varlen_reference(c, mask, columns=None):
    out = torch.zeros(c["q"].shape[0], c["q"].shape[1], c["DV"], dtype=torch.float64)
    v = varlen_v(c, c["v_wide"])
    for b, (Lq, Lk) in enumerate(zip(QLENS, KLENS)):
        qs, ks = int(c["cu_q"][b]), int(c["cu_k"][b])
        if Lq == 0:
            continue
        mult = mask(0, Lq, Lk)
        for j, n in (columns(0, Lq) if columns else {}).items():
            if j < Lk:
                mult[:, j] *= n
        out[qs:qs + Lq] = attend(c["q"][qs:qs + Lq].movedim(0, 1), c["k"][ks:ks + Lk].movedim(0, 1), v[ks:ks + Lk].movedim(0, 1),
                                 1.0 / c["q"].shape[2] ** 0.5, mult).movedim(0, 1)
    return out


@functools.lru_cache(maxsize=None)
def varlen_ref(D, DV, v_offset, is_causal):
    return varlen_reference(varlen_case(D, DV, v_offset), causal if is_causal else everything)


def run_varlen(ops, c, is_causal):
    q = c["q"].cuda()
    # the operator allocates its output: a NaN block of that size, freed just before, is what the caching allocator hands
    # back as a rule (best effort -- the finite check below means the most when it does)
    del_me = torch.full((q.shape[0], q.shape[1], c["DV"]), float("nan"), dtype=BF16, device="cuda")
    del del_me
    out = ops.flash_attn_varlen_func(q, c["k"].cuda(), varlen_v(c, c["v_wide"].cuda()), c["cu_q"].cuda(), c["cu_k"].cuda(),
                                     max(QLENS), max(KLENS), is_causal)
    assert out.shape == (q.shape[0], q.shape[1], c["DV"]) and out.dtype == BF16
    return out.cpu()


#            knobs               D    DV  v_offset
VARLEN = {
    "pp_128x128": ({}, 128, 128, 0),                          # two-phase varlen form: extend_pp_kernel<FORM 1>
    "pp0_128x128": ({"SGLK_ATTN_PP": 0}, 128, 128, 0),        # FA_CASE(128, 128) exact: extend_attention_kernel<128, 128, 2, FORM 1>
    "exact_64x64": ({}, 64, 64, 0),                           # FA_CASE(64, 64) exact: <64, 64, 2, 1>
    "exact_96x96": ({}, 96, 96, 0),                           # FA_CASE(96, 96) exact: <96, 96, 2, 1>
    "ragged_40x50": ({}, 40, 50, 0),                          # padded to 64 / 64, ragged: <64, 64, 2, FORM 2>
    "ragged_88x90": ({}, 88, 90, 0),                          # padded to 96 / 96, ragged: <96, 96, 2, 2>
    "v_rows_4_byte_aligned_128x128": ({}, 128, 128, 2),       # exact dims, only v_aligned fails: <128, 128, 2, 2>
}


@gpu
@pytest.mark.parametrize("is_causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("name", list(VARLEN))
def test_flash_attn_varlen_forms(ops, knob, name, is_causal):
    knobs, D, DV, v_offset = VARLEN[name]
    c, ref = varlen_case(D, DV, v_offset), varlen_ref(D, DV, v_offset, is_causal)
    knob(**knobs)
    out = run_varlen(ops, c, is_causal)
    report(name, ref, out)
    assert torch.isfinite(out.float()).all(), "a row was not written"
    assert extend_ok(ref, out), name


@gpu
@pytest.mark.parametrize("D,DV", [(32, 32), (128, 64)])
def test_flash_attn_varlen_rejects_head_dims_that_are_not_built(ops, D, DV):
    """Padded dims 32 / 32 and 128 / 64 have no FA_CASE: 'padded head dims not built'."""
    q = torch.zeros(8, 2, D, dtype=BF16, device="cuda")
    v = torch.zeros(8, 2, DV, dtype=BF16, device="cuda")
    cu = torch.tensor([0, 8], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="not built"):
        ops.flash_attn_varlen_func(q, q, v, cu, cu, 8, 8, True)


# ---- decode_attention_cpu --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decode_case(D, DV, HQ, HKV, alias, lens, qmul=1.0, cap=0.0, seed=0):
    """Page tables are a random permutation of the cache rows, `loc` is each request's last position.  The reference runs over
    the cache as it stands after the write (k_after / v_after)."""
    g = torch.Generator().manual_seed(3000 + seed)
    B, rows = len(lens), sum(lens) + 5
    perm = torch.randperm(rows, generator=g)
    rtt = torch.zeros(B, max(lens) + 3, dtype=torch.int64)
    for b, n in enumerate(lens):
        rtt[b, :n] = perm[sum(lens[:b]):sum(lens[:b]) + n]
    c = dict(D=D, DV=DV, HQ=HQ, HKV=HKV, alias=alias, lens=lens, cap=cap, scale=1.0 / D ** 0.5, q=randn(g, B, HQ, D, mul=qmul),
             k_buffer=randn(g, rows, HKV, D), key=randn(g, B, HKV, D), rtt=rtt,
             loc=torch.stack([rtt[b, n - 1] for b, n in enumerate(lens)]), seq=torch.tensor(lens), req=torch.arange(B))
    if not alias:
        c["v_buffer"], c["value"] = randn(g, rows, HKV, DV), randn(g, B, HKV, DV)
    c["k_after"] = c["k_buffer"].clone()
    c["k_after"][c["loc"]] = c["key"]
    if alias:                                    # v is k's first DV columns (MLA), and so is `value` of `key`
        c["v_after"] = c["k_after"][..., :DV]
    else:
        c["v_after"] = c["v_buffer"].clone()
        c["v_after"][c["loc"]] = c["value"]
    c["ref"] = decode_reference(c)
    return c


def decode_reference(c, cap=None, columns=None):
    out = torch.zeros(len(c["lens"]), c["HQ"], c["DV"], dtype=torch.float64)
    for b, L in enumerate(c["lens"]):
        toks = c["rtt"][c["req"][b], :L]
        mult = everything(0, 1, L)
        for j, n in (columns(L) if columns else {}).items():
            if j < L:
                mult[:, j] *= n
        out[b] = attend(c["q"][b].unsqueeze(1), c["k_after"][toks].movedim(0, 1), c["v_after"][toks].movedim(0, 1), c["scale"],
                        mult, c["cap"] if cap is None else cap).squeeze(1)
    return out


def run_decode(ops, c, depth):
    """-> output, k cache, v cache on the host; the output and the scratch start as NaN."""
    B, HQ, DV = len(c["lens"]), c["HQ"], c["DV"]
    kb, key = c["k_buffer"].cuda(), c["key"].cuda()
    vb, value = (kb[..., :DV], key[..., :DV]) if c["alias"] else (c["v_buffer"].cuda(), c["value"].cuda())
    o = torch.full((B, HQ, DV), float("nan"), dtype=BF16, device="cuda")
    logits = torch.full((B, HQ, depth, DV + 1), float("nan"), device="cuda")
    ops.decode_attention_cpu(c["q"].cuda(), kb, vb, o, key, value, c["loc"].cuda(), logits, c["rtt"].cuda(), c["req"].cuda(),
                             c["seq"].cuda(), c["scale"], c["cap"])
    return o.cpu(), kb.cpu(), vb.cpu()


# decode_attention_kernel<D, DV, V_ALIAS, ND, KH>: ND = 4 for groups (HQ / HKV) up to 16, 2 up to 32, else 1; KH = 2 for D >= 256
#           D    DV  HQ HKV alias  lengths        depth q*  cap
DECODE = {
    # DEC_CASE(192, 128) <192, 128, false, 4, 1>: split partials and merge; direct store (one split); a scratch 64 deep, where
    # per = ceil(seq / 64) leaves the trailing splits without a key
    "192x128_g4_depth8": (192, 128, 8, 2, False, (65, 300, 1), 8, 1.0, 0.0),
    "192x128_g4_depth1": (192, 128, 8, 2, False, (65, 300, 1), 1, 1.0, 0.0),
    "192x128_g4_depth64": (192, 128, 8, 2, False, (65, 300, 1), 64, 1.0, 0.0),
    "128x128_g24": (128, 128, 24, 1, False, (63, 130, 300), DEPTH, 1.0, 0.0),       # <128, 128, false, 2, 1>: ND = 2 not aliased
    "128x128_g40": (128, 128, 40, 1, False, (64, 65, 300), DEPTH, 1.0, 0.0),        # <128, 128, false, 1, 1>: third column tile half full
    "128x128_g64": (128, 128, 64, 1, False, (1, 63, 130), DEPTH, 1.0, 0.0),         # <128, 128, false, 1, 1>: the largest group
    "64x64_g33": (64, 64, 33, 1, False, (65, 130, 300), DEPTH, 1.0, 0.0),           # <64, 64, false, 1, 1>: one head in the third tile
    "mla_g16": (576, 512, 16, 1, True, (65, 200), DEPTH, 1.0, 0.0),                 # <576, 512, true, 4, 2>: a full column tile
    "mla_g40": (576, 512, 40, 1, True, (65, 200), DEPTH, 1.0, 0.0),                 # <576, 512, true, 1, 2>
    "mla_g64": (576, 512, 64, 1, True, (65, 200), DEPTH, 1.0, 0.0),                 # <576, 512, true, 1, 2>: all four column tiles
    "mla_g16_cap": (576, 512, 16, 1, True, (65, 200), DEPTH, 4.0, 30.0),            # the soft-cap on this operator
    "128x128_g24_cap": (128, 128, 24, 1, False, (63, 130, 300), DEPTH, 4.0, 30.0),
}


def decode_args(name):
    D, DV, HQ, HKV, alias, lens, depth, qmul, cap = DECODE[name]
    return decode_case(D, DV, HQ, HKV, alias, lens, qmul, cap, seed=D + HQ), depth


@gpu
@pytest.mark.parametrize("name", list(DECODE))
def test_decode_attention_forms(ops, name):
    c, depth = decode_args(name)
    out, kb, vb = run_decode(ops, c, depth)
    assert torch.equal(kb, c["k_after"]) and torch.equal(vb, c["v_after"]), "the cache after the write, bit for bit"
    report(name, c["ref"], out)
    assert decode_ok(c["ref"], out), name


@gpu
def test_decode_attention_rejects_a_group_of_65(ops):
    """More than 64 q heads per kv head have no column tile: RuntimeError before anything is written."""
    c = decode_case(128, 128, 65, 1, False, (63, 64, 65), seed=65)
    kb, vb = c["k_buffer"].cuda(), c["v_buffer"].cuda()
    o = torch.full((3, 65, 128), float("nan"), dtype=BF16, device="cuda")
    logits = torch.zeros(3, 65, DEPTH, 129, device="cuda")
    with pytest.raises(RuntimeError, match="at most 64 q heads per kv head"):
        ops.decode_attention_cpu(c["q"].cuda(), kb, vb, o, c["key"].cuda(), c["value"].cuda(), c["loc"].cuda(), logits,
                                 c["rtt"].cuda(), c["req"].cuda(), c["seq"].cuda(), c["scale"], 0.0)
    torch.cuda.synchronize()
    assert torch.equal(kb.cpu(), c["k_buffer"]) and torch.equal(vb.cpu(), c["v_buffer"])
    assert bool(o.isnan().all())


# ---- the tests must be able to fail ----------------------------------------------------------------------------------------
def swap_heads(ref, head_dim):
    """q heads 0 and 1 (one kv group in every case here) change places."""
    idx = torch.arange(ref.shape[head_dim])
    idx[0], idx[1] = 1, 0
    return ref.index_select(head_dim, idx)


def test_mutated_references_fail():
    """For one case of each family: a reference with one deliberate mistake must FAIL the family's predicate against the true
    reference -- else a kernel with that mistake would pass.  This is a condition on the inputs (lengths in the hundreds,
    randn data), not a measurement of any kernel, and it needs no GPU."""
    failed_to_fail = []

    def must_fail(ok, ref, mutant, what):
        assert ok(ref, ref.to(BF16)), f"{what}: the true reference must pass"
        if ok(ref, mutant.to(BF16)):
            failed_to_fail.append(f"{what} (relative rms {rel_rms(mutant, ref):.2e})")

    # extend: 64x64_two_query_blocks (prefix 130, 300 extend tokens); the soft-cap on cap_pp_128x128
    _, c = extend_args("64x64_two_query_blocks")
    ref = c["ref"]
    edge = lambda P, E: (P + KEYS - 1) // KEYS * KEYS        # first key of the first tile that holds extend tokens only
    for what, mutant in {
        "causal mask one key wider": extend_reference(c, mask=functools.partial(causal, shift=1)),
        "causal mask one key narrower": extend_reference(c, mask=functools.partial(causal, shift=-1)),
        "prefix one key short": extend_reference(c, columns=lambda P, E: {P - 1: 0}),
        "key dropped at a tile boundary": extend_reference(c, columns=lambda P, E: {edge(P, E): 0}),
        "key doubled at a tile boundary": extend_reference(c, columns=lambda P, E: {edge(P, E): 2}),
        "q heads swapped": swap_heads(ref, 1),
    }.items():
        must_fail(extend_ok, ref, mutant, "extend: " + what)
    _, c = extend_args("cap_pp_128x128")
    must_fail(extend_ok, c["ref"], extend_reference(c, cap=0.0), "extend: no logit_cap")

    # varlen: pp_128x128, causal
    c, ref = varlen_case(128, 128), varlen_ref(128, 128, 0, True)
    for what, mutant in {
        "causal mask one key wider": varlen_reference(c, functools.partial(causal, shift=1)),
        "causal mask one key narrower": varlen_reference(c, functools.partial(causal, shift=-1)),
        "key dropped at a tile boundary": varlen_reference(c, causal, columns=lambda P, E: {KEYS: 0}),
        "key doubled at a tile boundary": varlen_reference(c, causal, columns=lambda P, E: {KEYS: 2}),
        "q heads swapped": swap_heads(ref, 1),
    }.items():
        must_fail(extend_ok, ref, mutant, "varlen: " + what)
    must_fail(extend_ok, varlen_ref(128, 128, 0, False), ref, "varlen: causal where it should not be")

    # decode: 128x128_g24 (lengths 63, 130, 300 over 8 splits); the soft-cap on 128x128_g24_cap
    c, depth = decode_args("128x128_g24")
    ref = c["ref"]
    per = lambda L: (L + depth - 1) // depth                 # first key of the second split
    for what, mutant in {
        "sequence one key short": decode_reference(c, columns=lambda L: {L - 1: 0}),
        "key dropped at a split boundary": decode_reference(c, columns=lambda L: {per(L): 0}),
        "key doubled at a split boundary": decode_reference(c, columns=lambda L: {per(L): 2}),
        "q heads swapped": swap_heads(ref, 1),
    }.items():
        must_fail(decode_ok, ref, mutant, "decode: " + what)
    c, _ = decode_args("128x128_g24_cap")
    must_fail(decode_ok, c["ref"], decode_reference(c, cap=0.0), "decode: no logit_cap")

    assert not failed_to_fail, "mutants that pass: " + "; ".join(failed_to_fail)
