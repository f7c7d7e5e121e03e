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

}  // namespace soar
