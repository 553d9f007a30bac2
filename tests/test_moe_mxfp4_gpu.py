"""GPU parity of fused_experts with MX-fp4 (W4A16) expert weights, through fused_experts_cpu.method (method 4) -> C-ABI -> HIP.

Expected values: oracle.moe.fused_experts_f32 on the weights expanded by oracle.gemm.mxfp4_dequant (fp32).  Pass predicate:
tests/test_moe_fp8_gpu.py's check_close for a path with three bf16 roundings (ic1, the per-slot GEMM-2 row, the output).
Inputs are scaled like recipes.moe_fp8_inputs: hidden ~ randn / sqrt(K), weights ~ 0.45 randn (its fp8 weight x block scale).
"""
import math

import pytest
import torch

from oracle import gemm, moe

pytestmark = pytest.mark.gpu

E, TOPK, MXFP4 = 4, 2, 4
_CASES = {}   # (M, N, K, routing) -> inputs and the fp32 oracle's output, computed once


@pytest.fixture(scope="module")
def ops():
    import sgl_kernel  # noqa: F401
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.ops.sgl_kernel


def run(ops, M, N, K, routing="topk", is_vnni=False, inplace=False, row_pad=0):
    """One call on the seeded case (M, N, K, routing); returns (out, fp32 reference)."""
    key = (M, N, K, routing)
    if key not in _CASES:
        g = torch.Generator().manual_seed(4000 + M + N + K)
        a = (torch.randn(M, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
        w1, w1s = gemm.mxfp4_quantize(torch.randn(E, 2 * N, K, generator=g) * 0.45)
        w2, w2s = gemm.mxfp4_quantize(torch.randn(E, K, N, generator=g) * 0.45)
        tw, ids = torch.topk(torch.softmax(torch.randn(M, E, generator=g), dim=-1), TOPK)
        ids = ids.to(torch.int32)
        if routing == "skew":          # expert 0 gets 2 (M - 4) slots, expert 3 none
            ids[: M - 4] = 0
            ids[M - 4:] = torch.tensor([1, 2], dtype=torch.int32)
        elif routing == "masked":      # a third of the slots
            ids.view(-1)[::3] = -1
        elif routing == "all_masked":
            ids.fill_(-1)
        w1s, w2s = w1s.view(E, 2 * N, K // 32), w2s.view(E, K, N // 32)   # (the quantiser returns them as one column)
        ref = moe.fused_experts_f32(a, gemm.mxfp4_dequant(w1, w1s), gemm.mxfp4_dequant(w2, w2s), tw, ids)
        _CASES[key] = (dict(a=a, w1=w1, w2=w2, w1s=w1s, w2s=w2s, tw=tw.contiguous(), ids=ids.contiguous()), ref)
    inp, ref = _CASES[key]
    d = {k: v.cuda() for k, v in inp.items()}
    hidden = d["a"]
    if row_pad:                        # the same rows inside a wider buffer
        hidden = torch.zeros(M, K + row_pad, dtype=torch.bfloat16, device="cuda")[:, :K]
        hidden.copy_(d["a"])
    out = ops.fused_experts_cpu.method(hidden, d["w1"], d["w2"], d["tw"], d["ids"], inplace, MXFP4, d["w1s"], d["w2s"],
                                       None, None, None, is_vnni)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (M, K)
    assert M == 0 or (out.data_ptr() == hidden.data_ptr()) == bool(inplace)
    return out.cpu(), ref


def check(out, ref, what, tile=None):
    from sgl_kernel import _lib, _ops
    assert _ops.last_path & _lib.PATH_MXFP4, f"{what}: not the MX-fp4 path (0x{_ops.last_path:x})"
    if tile is not None:
        assert _ops.last_path & _lib.PATH_TILE_MASK == tile, f"{what}: tile {_ops.last_path & _lib.PATH_TILE_MASK}, expected {tile}"
    err = (out.float() - ref).norm() / ref.norm().clamp_min(1e-12)
    print(f"{what}: relative RMS error {err:.3e}, max |diff| {(out.float() - ref).abs().max():.3e}")
    assert torch.allclose(ref.bfloat16(), out, rtol=1e-2, atol=1e-2), f"{what}: reference predicate failed"
    assert err < 6e-3, f"{what}: relative RMS error {err:.2e}"


@pytest.mark.parametrize("tile", [32, 128])
@pytest.mark.parametrize("M,N,K,routing", [
    (1, 128, 128, "topk"),        # one slot per tile, one block per reduction
    (33, 384, 384, "topk"),       # odd number of 128-blocks in both reductions, three column tiles, partial 32-slot tiles
    (70, 128, 256, "skew"),       # 132 slots on one expert (five 32-slot tiles / crosses a 128-slot tile), one expert empty
    (40, 256, 128, "masked"),     # a third of the ids -1
])
def test_parity(ops, knob, M, N, K, routing, tile):
    knob(SGLK_MXFP4_MOE_TILE=tile)
    out, ref = run(ops, M, N, K, routing)
    check(out, ref, f"M={M} N={N} K={K} {routing} tile={tile}", tile)


def test_same_bits(ops):
    base, _ = run(ops, 40, 256, 128, "masked")
    for what, kw in [("is_vnni", dict(is_vnni=True)), ("second run", {}), ("padded rows", dict(row_pad=3)),
                     ("inplace on padded rows", dict(inplace=True, row_pad=3))]:
        out, _ = run(ops, 40, 256, 128, "masked", **kw)
        assert torch.equal(out, base), what


@pytest.mark.parametrize("M,tile", [(4, 32), (72, 128)])
def test_default_dispatch(ops, M, tile):
    out, ref = run(ops, M, 128, 128)
    check(out, ref, f"default M={M}", tile)


def test_all_masked_and_empty(ops):
    out, _ = run(ops, 5, 128, 128, "all_masked")
    assert torch.count_nonzero(out.float()) == 0
    out0, _ = run(ops, 0, 128, 128)
    assert tuple(out0.shape) == (0, 128)


@pytest.mark.parametrize("bad", ["K=192", "f32 scales", "w1 columns", "bf16 weights"])
def test_rejections(ops, bad):
    M, N, K = 4, 128, 192 if bad == "K=192" else 128
    a = torch.zeros(M, K, dtype=torch.bfloat16, device="cuda")
    w1 = torch.zeros(E, 2 * N, K // 2 + (bad == "w1 columns"), dtype=torch.uint8, device="cuda")
    w2 = torch.zeros(E, K, N // 2, dtype=torch.uint8, device="cuda")
    sdt = torch.float32 if bad == "f32 scales" else torch.uint8
    w1s = torch.zeros(E, 2 * N, K // 32, dtype=sdt, device="cuda")
    w2s = torch.zeros(E, K, N // 32, dtype=sdt, device="cuda")
    if bad == "bf16 weights":
        w1, w2 = torch.zeros(E, 2 * N, K, dtype=torch.bfloat16, device="cuda"), torch.zeros(E, K, N, dtype=torch.bfloat16, device="cuda")
    tw = torch.ones(M, TOPK, device="cuda")
    ids = torch.zeros(M, TOPK, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        ops.fused_experts_cpu.method(a, w1, w2, tw, ids, False, MXFP4, w1s, w2s, None, None, None, False)
