/*
 * gritlm_hip_index.h -- the 16-bit RAG index search of libgritlm_hip.so: a second header beside gritlm_hip.h, whose conventions
 * (device pointers + explicit sizes, `stream` = hipStream_t as void*, nothing allocates or synchronises, 0 / negative GRIT_E_*,
 * grit_last_error_string() explains, workspace queries return 0 for sizes the compute entry rejects) and error codes it shares.
 * It is separate only because the main header's symbol set is pinned by a recorded call trace; the entries move there when that
 * recording is next re-made.
 */
#ifndef GRITLM_HIP_INDEX_H
#define GRITLM_HIP_INDEX_H

#include <stddef.h>
#include <stdint.h>

#include "gritlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- RAG index search on a bf16 / fp16 index as it lies: rag/index.py:97-104 (scores = queries @ embeddings; torch.topk) with
 *      the index kept in --idxdtype bfloat16|float16 (rag/index.py:21,194, rag/eval.py:115,145) ------------------------------------ */

/* Exhaustive inner-product search.  queries [Q,H] fp32 (contiguous); embeddings: the reference's index layout [H,N] (index.py:141) of
 * 16-bit values -- bf16, or IEEE fp16 when is_f16 != 0 -- element (h,n) at h*ld + n, ld >= N, any 2-byte-aligned address (rows whose
 * starts are 16-byte aligned, i.e. ld % 8 == 0 and a 16-byte-aligned base, are staged with single full-width loads; the result bits
 * are the same either way).  The queries are NOT rounded to the index format: each is split exactly into three 16-bit pieces, every
 * MFMA product is exact, only the fp32 accumulation rounds.  The k best columns per query (descending, lower column first on equal
 * scores; a NaN score counts as -inf): out_scores [Q,k] fp32, out_index [Q,k] int64.  No [Q,N] score matrix exists: the selection is
 * fused into the scan, the workspace does not depend on N beyond the strip count (<= 1024).  Bit-reproducible; a query's result does not
 * depend on Q or on the other queries.
 * 1 <= k <= min(N, 1024), Q <= 65535, N < 2^31.  workspace: grit_knn16_workspace_bytes(Q, N, H, k) bytes of device memory
 *   (<= 2*1024*Q*k*12 + 8*Q*(H + 64) + 4096). */
int64_t grit_knn16_workspace_bytes(int Q, int64_t N, int H, int k);
int grit_knn16_topk(const float* queries, const void* embeddings, int is_f16, int Q, int64_t N, int H, int64_t ld, int k,
                    void* workspace, float* out_scores, int64_t* out_index, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GRITLM_HIP_INDEX_H */
