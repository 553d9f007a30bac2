// decode_attention_multi: Q new tokens per request against the paged bf16 KV cache in ONE pass over the cache rows
// (speculative decoding: the verify step of EAGLE / MTP drafts).
//
// The one-token kernel (attention.hip: decode_attention_kernel) gives a workgroup at most 64 MFMA columns and a column is "one q
// head of the one new token"; here a column is a (token, head) pair
//     c = t * group + g          t = 0 .. Q-1 (draft position), g = q head inside the kv head's group
// so the Q * group columns of a (request, kv head) share ONE stream of cache rows.  What differs from the one-token kernel:
//   * columns: a workgroup owns one block of 16 * CT columns (CT = 4 / NDV column tiles of 16: 1, 2 or 4 by the column count;
//     64 columns at the most, 32 on wide heads -- see the launcher), and ceil(Q * group / block) blocks ride in grid.y beside
//     the kv head.  A lane's q row, its output row and its partial row are addressed per column: row b * Q + t, head
//     kvh * group + g.
//   * limits: token t sits at position p = seq_len - Q + t and sees keys 0 .. p, so the column's limit is min(k_end, p + 1),
//     clamped at 0.  Core::tile masks per column already, and a column whose limit lies in front of the split's range keeps
//     m = -inf, l = 0: its partial is (0, lse = -inf), which the merge skips.  A token with p < 0 gets a row of zeros.
//   * cache rows are read non-temporal only with ONE column block: with several, the same rows are read by several
//     workgroups and are left to the default policy.
// The K/V staging is that of the one-token kernel: double-buffered LDS-DMA tiles, the ring of page-id tables fetched by DMA a
// step ahead, counted s_waitcnt and bare barriers (attention_internal.h: TileDma).  The waves are KH key halves x CT column
// tiles x NDV value slices, each with an online-softmax state of its own; the key halves meet once, through LDS.
// The cache write is kv_cache_write_kernel over the B * Q rows, launched before; partials and merge are decode's.
#include "attention_internal.h"
#include "knobs.h"

namespace sglk {
namespace attn {

struct MultiParams {
    const unsigned short *q, *k_buf, *v_buf;
    int64_t q_s0, q_s1, kb_s0, kb_s1, vb_s0, vb_s1;
    float* logits;          // [B * Q][HQ][logit_splits][DV+1]
    const void* req_to_token;
    int64_t rtt_stride;
    int rtt_is64;
    const int64_t* b_req_idx;
    const int64_t* b_seq_len;   // counts the Q new tokens
    int HQ, HKV, Q, ncb;        // ncb = column blocks per (request, kv head)
    int splits, logit_splits;   // splits used / depth of the caller's scratch
    float sm_scale, logit_cap;
    int nt;                 // cache rows are read non-temporal
    unsigned short* o;      // [B * Q][HQ][DV]
    int64_t o_s0, o_s1;
    int direct;             // one split: the kernel rounds and stores the output itself, no merge
};

template <int D, int DV, bool V_ALIAS, int NDV, int KH>
__global__ __launch_bounds__(256 * KH, 1) void decode_multi_kernel(const MultiParams p) {
    typedef TileDma<D, 256 * KH> DmaK;
    typedef TileDma<DV, 256 * KH> DmaV;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    constexpr int KB = kKeys * D * 2, VB = V_ALIAS ? 0 : kKeys * DV * 2;
    constexpr bool kDouble = 2 * (KB + VB) <= SGLK_DEC_DOUBLE_LIMIT;
    constexpr int DVW = DV / NDV, CT = 4 / NDV;
    constexpr int kDma = DmaK::N + (V_ALIAS ? 0 : DmaV::N);

    const int b = blockIdx.x, split = blockIdx.z;
    const int kvh = blockIdx.y / p.ncb, cb = blockIdx.y - kvh * p.ncb;
    const int group = p.HQ / p.HKV, ncol = p.Q * group;
    const int seq_raw = (int)p.b_seq_len[b];
    const int seq_len = seq_raw > 0 ? seq_raw : 0;
    const int per = (seq_len + p.splits - 1) / p.splits;
    const int k_begin = split * per;
    const int k_end = (k_begin + per < seq_len) ? k_begin + per : seq_len;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kh = KH == 2 ? wave >> 2 : 0, w4 = wave & 3;   // key half; (column tile, value slice) index
    const int ct = w4 / NDV, dsl = w4 - ct * NDV;
    const int col = (cb * CT + ct) * 16 + (lane & 15);   // (token, head) column of this lane
    const bool col_valid = col < ncol;
    const bool wave_active = (cb * CT + ct) * 16 < ncol;
    const int tq = col_valid ? col / group : 0;          // draft position
    const int h = kvh * group + (col_valid ? col - tq * group : 0);
    const int64_t row = (int64_t)b * p.Q + tq;           // row of q / o / the partials

    Core<D, DVW, 1> core;
    core.init();
    if (wave_active) core.load_q(0, col_valid ? p.q + row * p.q_s0 + (int64_t)h * p.q_s1 : nullptr, lane);
    // the token's own position is seq_len - Q + tq; it sees the keys up to and including it
    int vis = seq_len - p.Q + tq + 1;
    vis = vis < k_end ? vis : k_end;
    int limit[1] = {col_valid && vis > 0 ? vis : 0};

    const int64_t req = p.b_req_idx[b];
    KvSource ks, vs;
    const unsigned char* page = reinterpret_cast<const unsigned char*>(p.req_to_token) + req * p.rtt_stride * (p.rtt_is64 ? 8 : 4);
    ks.buf = p.k_buf + (int64_t)kvh * p.kb_s1; ks.buf_stride_tok = p.kb_s0; ks.page = page; ks.page_is64 = p.rtt_is64;
    ks.n_paged = seq_len; ks.ext = nullptr; ks.ext_stride_tok = 0;
    vs = ks;
    vs.buf = p.v_buf + (int64_t)kvh * p.vb_s1; vs.buf_stride_tok = p.vb_s0;
    const float scale_log2e = p.sm_scale * 1.4426950408889634f;

    // every row up to k_end is streamed, also where only the block's last token sees it: at most Q - 1 rows too many
    const int ntiles = k_end > k_begin ? (k_end - k_begin + kKeys - 1) / kKeys : 0;
    auto compute = [&](int t, const unsigned char* cur) {
        if (wave_active)
            core.template tile<V_ALIAS, DV, 4 / KH, true>(cur, V_ALIAS ? cur : cur + KB, k_begin + t * kKeys, limit, scale_log2e,
                                                          p.logit_cap, lane, dsl * DVW, kh * 32);
    };
    if constexpr (kDouble) {
        // Queue of a wave at the wait of tile t:  ... rows(t) | [ids(t+2)] rows(t+1)  -> s_waitcnt vmcnt(kDma) covers rows(t), ids(t+2)
        // (decode_attention_kernel: tile t+2's rows are requested the moment every wave has left tile t's buffer)
        static_assert(kDma <= 63, "the counted wait must fit s_waitcnt's vmcnt field");
        unsigned char* const buf0 = dyn_lds;
        unsigned char* const buf1 = dyn_lds + KB + VB;
        unsigned* const idring = reinterpret_cast<unsigned*>(dyn_lds + 2 * (KB + VB));   // 4 tables of 64 ids
        auto lookup = [&](int t) {
            if (wave != 0) return;
            const int tt = t < ntiles ? t : ntiles - 1;          // past the end: the last tile's ids again (never used)
            const int p0 = k_begin + tt * kKeys;
            const int nk = k_end - p0 < kKeys ? k_end - p0 : kKeys;
            DmaK::lookup_dma(idring + (t & 3) * kKeys, ks, p0, nk, lane);
        };
        auto issue_rows = [&](int t, unsigned char* buf) {
            const unsigned* ids = idring + (t & 3) * kKeys;
            if (p.nt) {
                DmaK::template issue_rows<2>(buf, ks, ids, wave, lane);
                if constexpr (!V_ALIAS) DmaV::template issue_rows<2>(buf + KB, vs, ids, wave, lane);
            } else {
                DmaK::template issue_rows<0>(buf, ks, ids, wave, lane);
                if constexpr (!V_ALIAS) DmaV::template issue_rows<0>(buf + KB, vs, ids, wave, lane);
            }
        };
        if (ntiles > 0) {
            lookup(0);
            lookup(1);
            lookup(2);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            issue_rows(0, buf0);
            if (ntiles > 1) issue_rows(1, buf1);
        }
        for (int t = 0; t < ntiles; ++t) {
            unsigned char* const cur = (t & 1) ? buf1 : buf0;
            if (t + 1 < ntiles) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kDma) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // bare s_barrier: __syncthreads()' fence would make the compiler drain vmcnt -- the rows in flight -- in front of it
            __builtin_amdgcn_s_barrier();         // every wave's share of tile t has landed, and the id table of tile t+2
            asm volatile("" ::: "memory");
            compute(t, cur);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();         // every wave has left `cur`
            asm volatile("" ::: "memory");
            if (t + 2 < ntiles) {
                lookup(t + 3);
                issue_rows(t + 2, cur);
            }
        }
    } else {   // one tile buffer (an unaliased 576 / 512 cache): per-lane page lookups, a tile per memory round trip
        auto issue = [&](int t) {
            const int p0 = k_begin + t * kKeys;
            const int nk = k_end - p0 < kKeys ? k_end - p0 : kKeys;
            DmaK::issue(dyn_lds, ks, p0, nk, wave, lane);
            if constexpr (!V_ALIAS) DmaV::issue(dyn_lds + KB, vs, p0, nk, wave, lane);
        };
        if (ntiles > 0) issue(0);
        for (int t = 0; t < ntiles; ++t) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            compute(t, dyn_lds);
            __syncthreads();                     // the single buffer is free again
            if (t + 1 < ntiles) issue(t + 1);
        }
    }
    (void)kDma;
    // ---- merge the two key halves: the upper half parks {o, m, l} lane for lane in LDS (the tile buffers are dead), the
    //      lower half rescales both to the common maximum and adds ----
    float lsum = core.column_sum(0);
    constexpr int XS = DVW / 4 + 2;                     // floats per lane: its o registers, m, l
    static_assert(KH == 1 || 4 * 64 * XS * 4 <= (kDouble ? 2 : 1) * (KB + VB), "the key halves are merged in the tile buffers");
    float* xch = reinterpret_cast<float*>(dyn_lds) + (size_t)(w4 * 64 + lane) * XS;
    if (KH == 2) __syncthreads();
    if (KH == 2 && kh == 1 && wave_active) {
#pragma unroll
        for (int t = 0; t < DVW / 16; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) xch[t * 4 + j] = core.o[0][t][j];
        xch[DVW / 4] = core.m[0];
        xch[DVW / 4 + 1] = lsum;
    }
    if (KH == 2) __syncthreads();
    if (kh == 1 || !wave_active) return;
    if (KH == 2) {
        const float m1 = xch[DVW / 4], l1 = xch[DVW / 4 + 1];
        const float m0 = core.m[0];
        const float mt = fmaxf(m0, m1);
        // a half that saw no visible key has m = -inf and contributes nothing (and exp2(-inf - -inf) must not be taken)
        const float a0 = (m0 == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m0 - mt);
        const float a1 = (m1 == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m1 - mt);
#pragma unroll
        for (int t = 0; t < DVW / 16; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) core.o[0][t][j] = core.o[0][t][j] * a0 + xch[t * 4 + j] * a1;
        lsum = lsum * a0 + l1 * a1;
        core.m[0] = mt;
    }
    if (!col_valid) return;
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;    // a column that sees no key of this split: zeros, lse = -inf
    const int g4 = (lane >> 4) * 4;
    if (p.direct) {
        unsigned short* orow = p.o + row * p.o_s0 + (int64_t)h * p.o_s1 + dsl * DVW + g4;
#pragma unroll
        for (int t = 0; t < DVW / 16; ++t) {
            const f32x4 v = core.o[0][t] * inv;
            uint2 w;
            w.x = pack_bf16x2(v[0], v[1]);
            w.y = pack_bf16x2(v[2], v[3]);
            *reinterpret_cast<uint2*>(orow + t * 16) = w;
        }
        return;
    }
    float* dst = p.logits + ((row * p.HQ + h) * p.logit_splits + split) * (DV + 1);
#pragma unroll
    for (int t = 0; t < DVW / 16; ++t) {
        const f32x4 v = core.o[0][t] * inv;
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[dsl * DVW + t * 16 + g4 + j] = v[j];
    }
    // log-sum-exp of the split in log2 units (m is in log2 units); -inf marks a split the column sees nothing of
    if (dsl == 0 && (lane >> 4) == 0) dst[DV] = lsum > 0.f ? core.m[0] + __builtin_amdgcn_logf(lsum) : -INFINITY;
}

template <int D, int DV, bool AL, int NDV>
static int launch_multi(const MultiParams& p, dim3 grid, hipStream_t s) {
    constexpr size_t kb = (size_t)kKeys * D * 2, vb = AL ? 0 : (size_t)kKeys * DV * 2;
    constexpr size_t lds = (2 * (kb + vb) <= SGLK_DEC_DOUBLE_LIMIT) ? 2 * (kb + vb) + 4 * kKeys * 4 : (kb + vb);   // + id tables
    constexpr int kh = D >= 256 ? SGLK_DEC_KH_WIDE : 1;   // wide heads: the tile's keys are split over two wave groups
    SGLK_ENSURE_DYN_LDS((decode_multi_kernel<D, DV, AL, NDV, kh>), lds, "decode_attention_multi");
    hipLaunchKernelGGL((decode_multi_kernel<D, DV, AL, NDV, kh>), grid, dim3(256 * kh), lds, s, p);
    SGLK_CHECK_LAUNCH("decode_attention_multi");
    return SGLK_OK;
}

// value slices by the column count: up to 16 columns are one column tile whose value width four waves share, up to 32 two
// tiles x two slices, more than that four tiles (one block of 64 columns per workgroup)
template <int D, int DV>
static int launch_by_columns(const MultiParams& p, bool alias, int ndv, dim3 grid, hipStream_t s) {
    if (alias) {
        if (ndv == 4) return launch_multi<D, DV, true, 4>(p, grid, s);
        if (ndv == 2) return launch_multi<D, DV, true, 2>(p, grid, s);
        return launch_multi<D, DV, true, 1>(p, grid, s);
    }
    if (ndv == 4) return launch_multi<D, DV, false, 4>(p, grid, s);
    if (ndv == 2) return launch_multi<D, DV, false, 2>(p, grid, s);
    return launch_multi<D, DV, false, 1>(p, grid, s);
}

}  // namespace attn
}  // namespace sglk

using namespace sglk;
using namespace sglk::attn;

extern "C" int sglk_decode_attention_multi(const sglk_decode_attention_multi_args* a, void* stream) {
    const char* const what = "decode_attention_multi";
    SGLK_REQUIRE(a, SGLK_ERR_INVALID, "%s: null args", what);
    SGLK_REQUIRE(a->B >= 0 && a->HQ > 0 && a->HKV > 0 && a->HQ % a->HKV == 0, SGLK_ERR_INVALID, "%s: bad head counts HQ=%d HKV=%d",
                 what, a->HQ, a->HKV);
    SGLK_REQUIRE(a->Q >= 1, SGLK_ERR_INVALID, "%s: Q=%d query tokens per request (need >= 1)", what, a->Q);
    SGLK_REQUIRE(a->splits > 0 && a->splits <= 64, SGLK_ERR_INVALID, "%s: attn_logits must have 1 .. 64 splits", what);
    SGLK_REQUIRE((a->D == 576 && a->DV == 512) || (a->D == 128 && a->DV == 128) || (a->D == 192 && a->DV == 128) ||
                     (a->D == 64 && a->DV == 64), SGLK_ERR_SHAPE,
                 "%s: head dims D=%d DV=%d not built (have 576/512, 128/128, 192/128, 64/64)", what, a->D, a->DV);
    if (a->B == 0) return SGLK_OK;
    SGLK_REQUIRE(a->q && a->k_buffer && a->v_buffer && a->o && a->key && a->value && a->loc && a->attn_logits && a->req_to_token &&
                     a->b_req_idx && a->b_seq_len, SGLK_ERR_INVALID, "%s: null pointer", what);
    for (int64_t st : {a->q_stride[0], a->q_stride[1], a->k_buffer_stride[0], a->k_buffer_stride[1], a->v_buffer_stride[0],
                       a->v_buffer_stride[1]})
        SGLK_REQUIRE(st % 8 == 0, SGLK_ERR_SHAPE, "%s: q/k/v strides must be multiples of 8 elements", what);
    for (const void* ptr : {a->q, (const void*)a->k_buffer, (const void*)a->v_buffer})
        SGLK_REQUIRE(((uintptr_t)ptr % 16) == 0, SGLK_ERR_SHAPE, "%s: q and the caches must be 16-byte aligned", what);
    const int group = a->HQ / a->HKV;
    const int64_t T = (int64_t)a->B * a->Q, ncol = (int64_t)a->Q * group;
    // <= 16 columns: one tile, four value slices; <= 32: two tiles, two slices; else narrow heads take blocks of 64 columns (four
    // tiles, the whole value width per wave).  Wide heads (D >= 256) stay on blocks of 32: the 64-column form of the 576 / 512
    // head holds a 128-register accumulator beside 72 registers of q and spills 244 bytes per lane.  Measured, MLA 16 heads x
    // Q = 4 = 64 columns, B = 64 x 4096 keys (profiles/decode_multi_ops.txt): one block of 64 0.213 ms, two blocks of 32 -- the
    // rows streamed twice -- 0.123 ms.  SGLK_DECM_WIDE_COLS=64 selects the 64-column form (A/B).
    const bool half_blocks = a->D >= 256 && knobs().decm_wide_cols != 64;
    const int ndv = ncol <= 16 ? 4 : (ncol <= 32 || half_blocks) ? 2 : 1;
    const int64_t ncb = ceil_div(ncol, 64 / ndv);
    SGLK_REQUIRE(T < (1ll << 31) && a->HKV * ncb <= 65535 && a->HQ <= 65535, SGLK_ERR_SHAPE,
                 "%s: B * Q = %lld rows, %lld column blocks per request do not fit the launch grid", what, (long long)T,
                 (long long)(a->HKV * ncb));
    hipStream_t s = (hipStream_t)stream;
    // V aliases K when it is the same storage with the same strides (MLA: v = k[..., :DV])
    const bool alias = a->v_buffer == a->k_buffer && a->v_buffer_stride[0] == a->k_buffer_stride[0] &&
                       a->v_buffer_stride[1] == a->k_buffer_stride[1] && a->DV <= a->D;
    // the write comes first and is a launch of its own: a page table may name any request's new rows
    int rc = launch_kv_cache_write(a->k_buffer, a->k_buffer_stride, a->v_buffer, a->v_buffer_stride, a->key, a->key_stride, a->value,
                                   a->value_stride, a->loc, a->loc_is64, (int)T, a->HKV, a->D, a->DV, s);
    if (rc != SGLK_OK) return rc;
    MultiParams p{};
    p.q = (const unsigned short*)a->q; p.k_buf = (const unsigned short*)a->k_buffer; p.v_buf = (const unsigned short*)a->v_buffer;
    p.q_s0 = a->q_stride[0]; p.q_s1 = a->q_stride[1]; p.kb_s0 = a->k_buffer_stride[0]; p.kb_s1 = a->k_buffer_stride[1];
    p.vb_s0 = a->v_buffer_stride[0]; p.vb_s1 = a->v_buffer_stride[1]; p.logits = a->attn_logits;
    p.req_to_token = a->req_to_token; p.rtt_stride = a->req_to_token_stride; p.rtt_is64 = a->req_to_token_is64;
    p.b_req_idx = a->b_req_idx; p.b_seq_len = a->b_seq_len; p.HQ = a->HQ; p.HKV = a->HKV; p.Q = a->Q; p.ncb = (int)ncb;
    // every (request, kv head, column block, split) is a workgroup: the column blocks count like kv heads
    const int eff = decode_effective_splits(a->B, (int)(a->HKV * ncb), a->D, a->splits);
    p.splits = eff;
    p.logit_splits = a->splits;
    p.sm_scale = a->sm_scale; p.logit_cap = a->logit_cap;
    // several column blocks read the same cache rows: only a lone block reads them non-temporal (SGLK_DEC_NT=0: never)
    p.nt = (knobs().dec_nt != 0 && ncb == 1) ? 1 : 0;
    p.o = (unsigned short*)a->o; p.o_s0 = a->o_stride[0]; p.o_s1 = a->o_stride[1];
    p.direct = (eff == 1 && a->o_stride[0] % 4 == 0 && a->o_stride[1] % 4 == 0 && ((uintptr_t)a->o % 8) == 0) ? 1 : 0;
    const dim3 grid((unsigned)a->B, (unsigned)(a->HKV * ncb), (unsigned)eff);
    if (a->D == 576) rc = launch_by_columns<576, 512>(p, alias, ndv, grid, s);
    else if (a->D == 128) rc = launch_by_columns<128, 128>(p, alias, ndv, grid, s);
    else if (a->D == 192) rc = launch_by_columns<192, 128>(p, alias, ndv, grid, s);
    else rc = launch_by_columns<64, 64>(p, alias, ndv, grid, s);
    if (rc != SGLK_OK || p.direct) return rc;
    return launch_decode_merge(a->attn_logits, a->o, a->o_stride[0], a->o_stride[1], (int)T, a->HQ, eff, a->splits, a->DV, s);
}
