// Pieces of decode attention (attention.hip) that the fp8-cache form (attention_fp8kv.hip) launches too.
#pragma once
#include "sglk_common.h"

namespace sglk {
namespace attn {

// KV splits decode attention uses out of the `splits` the caller's attn_logits scratch has room for (see the definition)
int decode_effective_splits(int B, int HKV, int D, int splits);

// combines the first `eff` per-split partials (O / l, log-sum-exp) of attn_logits [B][HQ][splits][DV + 1] into o (bf16)
int launch_decode_merge(const float* attn_logits, void* o, int64_t o_s0, int64_t o_s1, int B, int HQ, int eff, int splits, int DV,
                        hipStream_t stream);

}  // namespace attn
}  // namespace sglk
