#!/usr/bin/env python3
"""Developer tool: device time of fused_experts with MX-fp4 (W4A16) experts against the fp8 (W8A16) path of the same build, one process.

    python tools/probe_moe_mxfp4.py [M ...]          (default: 4 64 256 1024 4096 16384; Qwen3-30B-A3B experts: E 128, top-8, N 768, K 2048)

Every call of a timed window takes the next of four weight copies (2.4 GB fp8, 1.2 GB fp4), so no expert is re-read from a
cache that a served model would not have.  Up to 1024 tokens the number is a hipGraph replay (no host launch time in it); above,
events around back-to-back calls.  The MX-fp4 path is timed with its own tile choice and with each shape forced
(SGLK_MXFP4_MOE_TILE).  Weights are random bytes: the time does not depend on their values."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from bench_ops import graph_ms, ops, timed, torch  # noqa: E402
from sgl_kernel import _lib, _ops  # noqa: E402

E, TOPK, N, K, COPIES = 128, 8, 768, 2048, 4
Ms = [int(x) for x in sys.argv[1:]] or [4, 64, 256, 1024, 4096, 16384]
g = torch.Generator(device="cuda").manual_seed(11)
fp8, fp4 = [], []
for _ in range(COPIES):
    w1 = (torch.randn(E, 2 * N, K, device="cuda", generator=g) * 100).to(torch.float8_e4m3fn)
    w2 = (torch.randn(E, K, N, device="cuda", generator=g) * 100).to(torch.float8_e4m3fn)
    fp8.append((ops.convert_weight_packed(w1), ops.convert_weight_packed(w2),
                torch.rand(E, 2 * N // 128, K // 128, device="cuda", generator=g) * 1e-3,
                torch.rand(E, K // 128, N // 128, device="cuda", generator=g) * 1e-3))
    del w1, w2
    fp4.append((torch.randint(0, 256, (E, 2 * N, K // 2), device="cuda", generator=g, dtype=torch.uint8),
                torch.randint(0, 256, (E, K, N // 2), device="cuda", generator=g, dtype=torch.uint8),
                torch.randint(118, 124, (E, 2 * N, K // 32), device="cuda", generator=g, dtype=torch.uint8),
                torch.randint(118, 124, (E, K, N // 32), device="cuda", generator=g, dtype=torch.uint8)))


def device_ms(call, M):
    turn = [0]

    def fn(_=0):
        turn[0] += 1
        call(turn[0] % COPIES)
    return graph_ms(fn) if M <= 1024 else timed(fn, 40, warm=8)


print(f"# fused_experts, E={E} top-{TOPK} N={N} K={K}, device ms per call; mxfp4 columns: tile by size / forced 32 / forced 128")
print(f"# {'M':>6} {'fp8 W8A16':>10} {'path':>9} {'mxfp4':>9} {'tile':>5} {'tile 32':>9} {'tile 128':>9} {'fp8/mxfp4':>10}")
for M in Ms:
    x = (torch.randn(M, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
    tw, ids = torch.topk(torch.softmax(torch.randn(M, E, device="cuda", generator=g), dim=-1), TOPK)
    ids = ids.to(torch.int32)
    t8 = device_ms(lambda c: ops.fused_experts_cpu(x, fp8[c][0], fp8[c][1], tw, ids, False, False, True, fp8[c][2], fp8[c][3],
                                                   [128, 128], None, None, True), M)
    p8 = _ops.last_path
    t4 = {}
    for tile in (None, 32, 128):
        if tile is None:
            os.environ.pop("SGLK_MXFP4_MOE_TILE", None)
        else:
            os.environ["SGLK_MXFP4_MOE_TILE"] = str(tile)
        _lib.lib().sglk_reload_env()
        t4[tile] = device_ms(lambda c: ops.fused_experts_cpu.method(x, fp4[c][0], fp4[c][1], tw, ids, False, _ops.MXFP4_W4A16,
                                                                     fp4[c][2], fp4[c][3], None, None, None, False), M)
        if tile is None:
            chosen = _ops.last_path & _lib.PATH_TILE_MASK
    print(f"  {M:>6} {t8:>10.4f} {p8:>#9x} {t4[None]:>9.4f} {chosen:>5} {t4[32]:>9.4f} {t4[128]:>9.4f} {t8 / t4[None]:>10.2f}", flush=True)
