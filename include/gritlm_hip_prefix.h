/*
 * gritlm_hip_prefix.h -- decode attention over ONE shared copy of a prefix: a third header beside gritlm_hip.h, whose conventions
 * (device pointers + explicit sizes, `stream` = hipStream_t as void*, nothing allocates or synchronises, 0 / negative GRIT_E_*,
 * grit_last_error_string() explains, workspace queries return 0 for sizes the compute entries reject) and error codes it shares.
 * It is separate for the reason gritlm_hip_index.h is: the main header's symbol set is pinned by a recorded call trace.
 *
 * The setting (MistralDecoder.generate(do_sample=True, num_return_sequences=n, share_prefix=True)): B0 sequences, each continued by n
 * rows; row r = s*n + j belongs to sequence s = r / n.  Everything before the first sampled token -- cached document + prompt -- is
 * the PREFIX of a sequence, stored once: prefix_k / prefix_v [B0, nkv, Lpre, 128], rows 0 .. plen[s]-1 valid.  What a row generates
 * itself goes to its TAIL: tail_k / tail_v [B, nkv, Ltail, 128], B = B0*n, Ltail a multiple of 64.  lens[r] is the row's global
 * position (plen[s] + tokens generated so far): the new token of row r is rotated at position lens[r] and appended at tail slot
 * lens[r] - plen[s]; the row then attends to prefix keys 0 .. plen[s]-1 and tail keys 0 .. lens[r] - plen[s].
 * head_dim 128, nq / nkv <= 8.  f16 != 0: the fp16-operand formats of the decode step (the q|k|v row is fp32, K / V and ctx are fp16).
 *
 * One step of a layer is four launches (2 and 3 are independent of each other; the kernel boundary is the only hand-over):
 *   1. grit_rope_kv_append_tail          RoPE of q and k, k / v -> the row's tail
 *   2. grit_attn_decode_prefix           the n*gq query rows of a (sequence, kv head) against its prefix keys on the MFMA,
 *                                        chunks of grit_attn_decode_prefix_kc() keys per workgroup -> partials
 *   3. grit_attn_decode_tail             each row against its own tail, 64-key splits -> partials
 *   4. grit_attn_decode_prefix_combine   partials -> ctx
 *
 * The workspace holds, per (row r, query head h), nslot = ceil(Lpre / KC) + Ltail / 64 records of 130 floats at
 * ((r*nq + h)*nslot + slot)*130: (m, l, O[128]) with the NATURAL exponent convention -- m is a reference maximum of the scaled
 * scores s = scale * q.k, l = sum exp(s - m), O = sum exp(s - m) v, unnormalised fp32; an empty chunk or split holds the neutral
 * element (-inf, 0, 0).  Prefix chunks come first (slot c: keys c*KC .. c*KC+KC-1), then the tail splits.  (The prefix launch runs
 * its softmax in base 2 like every MFMA attention kernel here and converts m once when it stores a record; its m may lie up to
 * 8 ln 2 below the chunk's true maximum -- the deferred rescale of attn_tile.h -- with l and O consistent with it.)
 * A row's result depends only on its own q, its sequence's prefix and its tail: not on n, B0 or the other rows (KC is a compile-time
 * constant).  The prefix products round P -- and, f16, q -- to the 16-bit operand format, as the encoder and prefill attention do.
 */
#ifndef GRITLM_HIP_PREFIX_H
#define GRITLM_HIP_PREFIX_H

#include <stddef.h>
#include <stdint.h>

#include "gritlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* keys per prefix chunk (a compile-time constant of the library, a multiple of 64) */
int grit_attn_decode_prefix_kc(void);

/* floats of workspace for B = B0*n rows; 0 for sizes the launches reject (Lpre <= 0, Ltail % 64, more than 512 records per row-head) */
int64_t grit_attn_decode_prefix_workspace_floats(int B, int nq, int nkv, int Lpre, int Ltail);

/* qkv [B, qkv_stride]: the fused q|k|v row of every row's new token (bf16; f16: fp32).  q is rotated in place at position lens[r]
 * (bf16: one rounding; f16: fp32, and q16 [B, q16_stride] receives the fp16 rounding of the rotated q heads -- the MFMA operand of
 * launch 2; q16 is NULL for bf16), k rotated and v are written to tail slot lens[r] - plen[r / n] (f16: rounded to fp16 once; a
 * non-finite k, v or q16 value sets the fp16 overflow flag).  cos / sin [Lpos, 64] fp32.  A row whose slot lies outside
 * [0, Ltail) or whose position is >= Lpos is left alone. */
int grit_rope_kv_append_tail(void* qkv, const float* cos_tab, const float* sin_tab, void* tail_k, void* tail_v, const int32_t* lens,
                             const int32_t* plen, void* q16, int B, int n, int nq, int nkv, int d, int Ltail, int Lpos,
                             int64_t qkv_stride, int64_t q16_stride, int f16, void* stream);

/* q [B0*n, q_stride] 16-bit rows whose first nq*128 columns are the rotated q heads (bf16: the q|k|v rows; f16: q16 above).
 * Writes the prefix records of every (row, head): chunk c covers keys c*KC .. min(c*KC + KC, plen[s]) - 1; nothing at or past
 * plen[s] is read. */
int grit_attn_decode_prefix(const void* q, const void* prefix_k, const void* prefix_v, const int32_t* plen, float* workspace, int B0,
                            int n, int nq, int nkv, int d, int Lpre, int Ltail, int64_t q_stride, float scale, int f16, void* stream);

/* q [B, q_stride]: the rotated q|k|v rows (bf16; f16: fp32).  Writes the tail records of every (row, head): split j covers tail keys
 * 64j .. min(64j + 64, lens[r] - plen[r / n] + 1) - 1, fp32 arithmetic (the form of grit_attn_decode). */
int grit_attn_decode_tail(const void* q, const void* tail_k, const void* tail_v, const int32_t* lens, const int32_t* plen,
                          float* workspace, int B, int n, int nq, int nkv, int d, int Lpre, int Ltail, int64_t q_stride, float scale,
                          int f16, void* stream);

/* out [B, out_stride] (bf16; f16: fp16): columns 0 .. nq*128-1 of row r = the normalised merge of the row's records. */
int grit_attn_decode_prefix_combine(const float* workspace, void* out, int B, int nq, int nkv, int d, int Lpre, int Ltail,
                                    int64_t out_stride, int f16, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRITLM_HIP_PREFIX_H */
