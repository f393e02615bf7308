/*
 * rip_head.h — extension of librip_hip.so's C ABI (rip_hip.h): the density head of K ensemble members trained on
 * cached encoder features, all members in one call.
 *
 * Members of a RIP ensemble are adapted by fine-tuning the head on a frozen encoder.  The head is ImitativeModel's
 * `_merger` (133 -> 64 -> 64 -> 64, ReLU after every layer, dim/model.py:56-61) and `_decoder` (GRUCell(2, 64) +
 * 64 -> 32 -> 4, torch/networks/sequence.py:53-65): RIP_HEAD_NUMEL floats, the contiguous tail of the packed vector
 * rip_load_model consumes (the last ten tensors of the reference's state_dict, in its order).  With the encoder in
 * eval mode its output feat [128] per (member, observation) is a constant — rip_encode writes it on request
 * (`feat_dev`) — so a training row is 128 + 5 + 8 floats and nothing of the encoder runs.
 *
 * Conventions are rip_hip.h's: 0 or a negative RIP_E* code, rip_last_error() for the message, validation before any
 * launch, caller-owned device memory, kernels enqueued on `stream` without synchronising, no allocation.  The entry
 * points are stateless and launch on the device that owns `head_dev`.  The optimizer step is rip_train_adam on the
 * flattened [K * RIP_HEAD_NUMEL] vectors with trainable_dev == NULL.
 *
 * This header has its own version: rip_abi_version() and the entry points of rip_hip.h are unchanged by it.
 */
#ifndef RIP_HEAD_H_
#define RIP_HEAD_H_

#include "rip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RIP_HEAD_ABI_VERSION 1
#define RIP_HEAD_NUMEL 32164
#define RIP_HEAD_FEATURES 128

int rip_head_abi_version(void);

/* Floats of one member's head (RIP_HEAD_NUMEL). */
size_t rip_head_numel(void);

/* Bytes of the workspace a gradient call on K members and up to max_batch rows needs (the per-row records whose outer
 * products are the weight gradients); 0 for arguments outside K in [1, RIP_MAX_MODELS], max_batch >= 1. */
size_t rip_head_workspace_bytes(int K, int max_batch);

/* Forward and (grads_dev != NULL) backward of the K heads on B rows each, three launches whatever K and B (two
 * without gradients):
 *   head_dev [K, RIP_HEAD_NUMEL]   the members' heads (16-byte aligned),
 *   feat_dev [K, n, 128], vec_dev [n, 5]   the cached encoder features and vector inputs of n observations,
 *   rows_dev [K, B] int64 or NULL  per member the cache rows of its batch (repeats allowed: a bootstrap sample or a
 *                                  shuffled epoch needs no batch-assembly launch); NULL = rows 0 .. B - 1 (n == B).
 *                                  A row outside [0, n) gives NaN in q_rows / z for that (member, row), a NaN loss
 *                                  and NaN gradients for that member, and touches no other member.
 *   target: y_dev [K, B, 4, 2] dense, or future_dev [n, L, 2] gathered as future[row, 0::stride] (the caller's L
 *           and stride must give RIP_T steps: stride >= 1, (L + stride - 1) / stride == RIP_T) plus the optional
 *           noise_dev [K, B, 4, 2].  Exactly one of y_dev / future_dev; noise_dev only with future_dev.
 * Per row: merged = cat(feat, vec), z = the merger's output (after its last ReLU), the teacher-forced inverse of the
 * flow (sequence.py:153-216), q = log_prob - logabsdet.  Outputs: q_rows_dev [K, B], loss_dev [K] = -mean_b q, z_dev
 * [K, B, 64] (may be NULL) and grads_dev [K, RIP_HEAD_NUMEL] = dloss_k / dhead_k (every element is written).
 * Gradient calls need workspace_dev of rip_head_workspace_bytes(K, max_batch) bytes, B <= max_batch; the sums over
 * the rows are added in an order fixed by B alone (no atomics): the same bits on every run, and member k's results
 * do not depend on K.  ReLU's derivative at 0 is 0 (torch's). */
int rip_head_forward_backward(const float* head_dev, float* grads_dev, const float* feat_dev, const float* vec_dev,
                              int64_t n, const int64_t* rows_dev, const float* y_dev, const float* future_dev, int L,
                              int stride, const float* noise_dev, int K, int B, int max_batch, void* workspace_dev,
                              float* q_rows_dev, float* loss_dev, float* z_dev, rip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RIP_HEAD_H_ */
