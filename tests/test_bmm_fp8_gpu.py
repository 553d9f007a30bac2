"""GPU parity of bmm_cpu with a float8_e4m3fn mat2 and a per-tensor scale (sglk_bmm_heads_fp8) against plain torch float64:
out = bf16(scale * mat1 @ float(mat2)^T), row-major and convert_weight_packed mat2, out / mat1 as transposed, narrowed views."""
import pytest
import torch

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def ops():
    import sgl_kernel  # noqa: F401
    assert torch.cuda.is_available()
    return torch.ops.sgl_kernel


def views(B, M, N, K, chunk, mat1):
    """mat1 and a NaN-filled out as transposed (and, with chunk, narrowed) device views, plus out's whole buffer."""
    pad = 64 if chunk else 0
    a = torch.zeros(M, B, K + pad, dtype=torch.bfloat16, device="cuda").narrow(2, 0, K).transpose(0, 1).copy_(mat1)
    buf = torch.full((M, B, N + pad), float("nan"), dtype=torch.bfloat16, device="cuda")
    return a, buf.narrow(2, 0, N).transpose(0, 1), buf


CASES = [(3, 7, 40, 72, False), (1, 5, 96, 160, True), (2, 17, 64, 128, True), (2, 70, 80, 192, True),
         (17, 111, 160, 544, True), (16, 1, 512, 128, True), (16, 33, 128, 512, True)]


@pytest.mark.parametrize("B,M,N,K,chunk", CASES)
def test_bmm_fp8(ops, B, M, N, K, chunk):
    g = torch.Generator().manual_seed(1000 * M + N + K)
    mat1 = torch.randn(B, M, K, generator=g).bfloat16()
    w = torch.randn(B, N, K, generator=g)
    amax = w.abs().max()
    q = (w * 448 / amax).clamp(-448, 448).to(FP8)
    scale = (amax / 448).float()
    ref = torch.bmm(mat1.double(), q.double().transpose(1, 2)) * scale.double()
    mag = torch.bmm(mat1.abs().double(), q.double().abs().transpose(1, 2)) * scale
    ref_bf16 = torch.bmm(mat1, q.to(torch.bfloat16).transpose(1, 2)) * scale     # the reference operator's own formulation
    a, out, buf = views(B, M, N, K, chunk, mat1)
    qd, sd = q.cuda(), scale.cuda()
    assert ops.bmm_cpu(out, a, qd, False, sd) is None
    got = out.cpu()
    err, bound = (got.double() - ref).abs(), 2.0 ** -8 * ref.abs() + 2.0 ** -14 * mag
    print(f"max |err| / bound = {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    assert torch.allclose(ref_bf16, got, rtol=1e-2, atol=1e-2)
    first = out.clone()
    out.fill_(float("nan"))
    ops.bmm_cpu(out, a, ops.convert_weight_packed(qd), True, sd)
    assert torch.equal(first, out), "packed and row-major mat2 must give the same bits"
    assert bool(buf[:, :, N:].isnan().all()), "nothing may be stored past N"


@pytest.mark.parametrize("packed", [False, True])
def test_bmm_fp8_identity_is_exact(ops, packed):
    B, K, N = 2, 128, 64 if packed else 48
    g = torch.Generator().manual_seed(7)
    bits = torch.randint(0, 256, (B, N, K), generator=g, dtype=torch.uint8)
    bits[(bits & 0x7F) == 0x7F] = 0x38          # the two NaN encodings -> 1.0
    q = bits.view(FP8).cuda()
    a = torch.eye(K, dtype=torch.bfloat16, device="cuda").expand(B, K, K).contiguous()
    out = torch.full((B, K, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops.bmm_cpu(out, a, ops.convert_weight_packed(q) if packed else q, packed, torch.tensor(0.25, device="cuda"))
    assert torch.equal(out.float(), q.float().transpose(1, 2) * 0.25)


def test_bmm_fp8_unaligned_views_give_the_same_bits(ops):
    """mat1 / out at 2-byte aligned pointers with odd strides take the element-wise load and store loops."""
    B, M, N, K = 2, 19, 40, 72
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, N, K, generator=g).mul(100).clamp(-448, 448).to(FP8).cuda()
    a0 = torch.randn(B, M, K, generator=g).bfloat16().cuda()
    s = torch.tensor(0.3, device="cuda")
    want = torch.empty(B, M, N, dtype=torch.bfloat16, device="cuda")
    ops.bmm_cpu(want, a0, q, False, s)
    a = torch.zeros(B, M, K + 3, dtype=torch.bfloat16, device="cuda")[:, :, 1:K + 1].copy_(a0)
    buf = torch.full((B, M, N + 3), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops.bmm_cpu(buf[:, :, 1:N + 1], a, q, False, s)
    assert torch.equal(buf[:, :, 1:N + 1], want)
    assert bool(buf[:, :, 0].isnan().all()) and bool(buf[:, :, N + 1:].isnan().all())


def test_bmm_fp8_rejects_bad_arguments(ops):
    def call(K=64, scale=torch.ones(1)):
        a = torch.zeros(2, 3, K, dtype=torch.bfloat16, device="cuda")
        w = torch.zeros(2, 32, K, dtype=torch.bfloat16, device="cuda").to(FP8)
        out = torch.zeros(2, 3, 32, dtype=torch.bfloat16, device="cuda")
        ops.bmm_cpu(out, a, w, False, None if scale is None else scale.cuda())

    call()
    for kw in (dict(scale=None), dict(scale=torch.ones(1).bfloat16()), dict(scale=torch.ones(2)), dict(K=68)):
        with pytest.raises(RuntimeError):
            call(**kw)
