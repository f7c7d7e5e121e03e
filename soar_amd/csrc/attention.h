// attention.h -- the two tiled multi-head attentions of the transformers (attention.hip).
#pragma once

#include "soar_common.h"

namespace soar {

constexpr int ATTN_SIDE = 64;          // grid attention: the longest side of a sequence (a window or the grid)

// SAM's grid attention (sam_attn_kernel): qkv [B][gh][gw][3 heads hd] -> out [B][gh][gw][heads hd], windows of win x win tokens (0: the
// whole grid is one sequence), the decomposed relative-position bias from rel_h / rel_w (or NULL both); bias: the qkv projection's,
// which is what a window's padding projects to.
int launch_sam_attention(const float *qkv, const float *bias, const float *rel_h, const float *rel_w, float *out, int B, int gh, int gw,
                         int heads, int hd, int win, float scale, hipStream_t stream);

// Separate query, key and value sources, any number of keys, an optional second key / value set (kv_attn_kernel).  hd_max: the widest
// head the caller's network may ask for (64 or 96); causal: one key set, Lq = Lk, key j counts for query i when j <= i.
int launch_kv_attention(const SoarUnetAttnArgs &a, int hd_max, bool causal, const char *me, hipStream_t stream);

// The same attention on the 16-bit matrix core (kv_attn16_kernel).  type: 1 bf16, 2 f16 (conv_gemm.h's WT_*); anything
// else is refused, as is everything launch_kv_attention refuses, before any launch.  The contract, T the type:
//   q, k, v, out and everything else in memory are float32;
//   q * scale is computed in float32 and then rounded to T, nearest even; k and v are rounded to T, nearest even, as their tile is
//   written to LDS;
//   S^T = K Q^T runs on v_mfma_f32_32x32x16_{bf16,f16} with float32 accumulation;
//   the masks, the running maximum m, corr, p = expf(s - m) and the running sum l are float32 exactly as in launch_kv_attention's
//   kernel, and l sums the UNROUNDED p;
//   p is rounded to T, nearest even, only as the operand of O^T += V^T P^T, which accumulates in float32;
//   1 / l, the w2 combination and the store are float32.
// Operands that overflow or are denormal in T are outside the contract.  No atomics; a (batch, head, query tile)'s result does not
// depend on the rest of the launch, and two runs give the same bits.
int launch_kv_attention16(const SoarUnetAttnArgs &a, int type, int hd_max, bool causal, const char *me, hipStream_t stream);
// type 0: launch_kv_attention; 1 / 2: launch_kv_attention16 (a network's attention_precision)
int launch_attention(const SoarUnetAttnArgs &a, int type, int hd_max, bool causal, const char *me, hipStream_t stream);

}  // namespace soar
