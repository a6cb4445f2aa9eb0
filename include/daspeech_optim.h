/* daspeech_optim.h — C ABI of the optimizer half of the fp16 training step (libdaspeech_hip.so): fairseq's FP16Optimizer with its fused Adam
 * (fairseq/optim/fp16_optimizer.py:111-211, fairseq/optim/adam.py:195-198) as two passes over a multi-tensor problem — the norm of the 16-bit
 * gradients, then unscale + clip + decoupled decay + Adam on the flat fp32 state + the 16-bit parameters, with no flat fp32 gradient between.
 * Conventions as in daspeech_dag.h (device pointers, caller-allocated outputs, hipStream_t as void*, int return codes).
 *
 * The problem (shared by both entries): N tensors of 16-bit data (dtype code DSP_F16 or DSP_BF16), each contiguous.
 *   grads    [N] device table of gradient pointers, any 2-byte-aligned address; NULL = this tensor has no gradient this step (g = 0)
 *   params16 [N] device table of the 16-bit parameter pointers, any 2-byte-aligned address
 *   offsets  [N] device table (int64): first element of tensor i in the three flat fp32 arrays master / exp_avg / exp_avg_sq, whose BASES
 *            are 16-byte aligned; a segment may start at any element
 *   items    [n_items][3] device table (int64): tensor index, first element within the tensor, count (1 .. chunk).  The items cover
 *            every element exactly once and none crosses a tensor.  One workgroup serves one item.
 *   chunk    a multiple of 2048, at most 65536: the largest count of an item
 * The fp32 streams move as 16-byte accesses wherever an item reaches a flat index that is a multiple of 4 (a peeled head of at most three
 * elements and a tail of at most three go one element at a time); the 16-bit side of a group of four moves as 8, 2 x 4 or 4 x 2 bytes,
 * by its address.  Cut the items at multiples of chunk in FLAT index space and the peeled head is empty except at a tensor's start. */
#ifndef DASPEECH_OPTIM_H
#define DASPEECH_OPTIM_H

#include "daspeech_dag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of dsp_fp16_optim_grad_sumsq for n_items work items: one fp32 partial per item.  Host arithmetic only; a multiple of 16,
 * 0 for n_items <= 0, monotone in n_items. */
size_t dsp_fp16_optim_workspace_bytes(int64_t n_items);

/* S = sum over every element of float(g)^2, one device double.
 *   Pass 1: the workgroup of item k writes partial[k] (fp32) = the sum of its squares in a fixed order that depends on the item alone (not
 *   on the address of the gradient); an item of a NULL gradient writes 0.  Pass 2: one workgroup adds the partials in double, every thread
 *   its items in ascending order, the threads' sums in ascending thread order.  No atomics: equal inputs give equal bits.  An inf or NaN
 *   gradient makes S non-finite — the overflow signal.
 *   N == 0 or n_items == 0: DSP_OK, nothing launched, S not written.  DSP_EINVAL: null grads / items / workspace / S, dtype, chunk off its
 *   grid.  DSP_ENOSPC: workspace_bytes < dsp_fp16_optim_workspace_bytes(n_items). */
int dsp_fp16_optim_grad_sumsq(const void* const* grads, int dtype, int N, const int64_t* items, int64_t n_items, int chunk,
                              void* workspace, size_t workspace_bytes, double* S, dsp_stream_t stream);

/* One Adam step with decoupled weight decay on the flat state, per element in fp32:
 *     g  = c * float(g16)                               (0 without a gradient)
 *     p  = p * (1 - lr_wd)
 *     m  = beta1 * m + (1 - beta1) * g
 *     v  = beta2 * v + (1 - beta2) * g * g
 *     p  = p - (lr / bias1) * m / (sqrt(v) / sqrt_bias2 + eps)          bias1 = 1 - beta1^t, sqrt_bias2 = sqrt(1 - beta2^t)
 *     master, exp_avg, exp_avg_sq <- p, m, v;  params16 <- round-to-nearest-even(p)
 *   The scalars are computed by the caller in double and passed as double: the entry derives 1 - beta1, 1 - beta2, 1 - lr_wd and lr / bias1
 *   in double and hands the kernel the float roundings (1 - beta2 taken from a float beta2 would be off by up to 3e-5 of itself, and
 *   exp_avg_sq with it).  The kernel's arithmetic is fp32.
 *   N == 0 or n_items == 0: DSP_OK, nothing launched.  DSP_EINVAL: a null table or flat array, dtype, a flat base off 16 bytes, chunk off
 *   its grid, t < 1, a beta outside [0, 1). */
int dsp_fp16_optim_adam_step(const void* const* grads, void* const* params16, int dtype, const int64_t* offsets, int N,
                             const int64_t* items, int64_t n_items, int chunk, float* master, float* exp_avg, float* exp_avg_sq,
                             double c, double lr, double beta1, double beta2, double eps, double lr_wd, double bias1, double sqrt_bias2,
                             int t, dsp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
