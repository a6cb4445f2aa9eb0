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

/* ---- The step without a host read: the decisions above made on the device.
 *
 * The optimizer state: DSP_OPTIM_STATE_SLOTS slots of 8 bytes in device memory, 8-byte aligned, doubles and int64s side by side (a 4-byte
 * field sits in the low half of its slot; the other half is not touched).  The caller initialises it once; afterwards
 * dsp_fp16_optim_scale_step owns every slot but the two inputs, which the host may rewrite between steps (stream-ordered writes).
 *   scaler and step
 *     LOSS_SCALE          double   the dynamic loss scale
 *     LOSS_SCALE_F32      float    the same value as a float: what a backward multiplies the loss by
 *     ITER                int64    steps seen, applied or skipped (starts at 0)
 *     LAST_OVERFLOW_ITER  int64    ITER of the last skipped step (starts at -1)
 *     T                   int64    applied steps (starts at 0)
 *     POW1, POW2          double   beta1^T, beta2^T as running products (start at 1.0)
 *   inputs
 *     LR                  double   learning rate
 *     GRAD_MULT           double   the factor the gradients are multiplied by beside 1 / LOSS_SCALE
 *   outputs of the last step
 *     GRAD_NORM           double   norm of the unscaled gradient before clipping; NaN or +inf on an overflow
 *     APPLIED             int32    1: the step is applied, 0: skipped on an overflow
 *     FLOOR_HIT           int32    sticky: set once LOSS_SCALE <= min_loss_scale after an overflow
 *     SCALARS             DSP_OPTIM_N_SCALARS floats from this slot on, packed: c, beta1, beta2, eps, 1 - lr*wd, lr / bias1, 1 - beta1,
 *                         1 - beta2, sqrt_bias2 — what the Adam kernel reads (valid when APPLIED == 1) */
#define DSP_OPTIM_SLOT_LOSS_SCALE 0
#define DSP_OPTIM_SLOT_LOSS_SCALE_F32 1
#define DSP_OPTIM_SLOT_ITER 2
#define DSP_OPTIM_SLOT_LAST_OVERFLOW_ITER 3
#define DSP_OPTIM_SLOT_T 4
#define DSP_OPTIM_SLOT_POW1 5
#define DSP_OPTIM_SLOT_POW2 6
#define DSP_OPTIM_SLOT_LR 7
#define DSP_OPTIM_SLOT_GRAD_MULT 8
#define DSP_OPTIM_SLOT_GRAD_NORM 9
#define DSP_OPTIM_SLOT_APPLIED 10
#define DSP_OPTIM_SLOT_FLOOR_HIT 11
#define DSP_OPTIM_SLOT_SCALARS 12
#define DSP_OPTIM_N_SCALARS 9
#define DSP_OPTIM_STATE_SLOTS 17

/* The state update of one step, one thread, in double.  S is the device double dsp_fp16_optim_grad_sumsq wrote on the same stream.
 *     c  = GRAD_MULT / LOSS_SCALE
 *     nv = (S == S && S >= 0) ? fabs(c) * sqrt(S) : NaN                                  -> GRAD_NORM
 *     nv NaN or +inf:  LAST_OVERFLOW_ITER = ITER; LOSS_SCALE /= scale_factor; ITER += 1;
 *                      FLOOR_HIT |= (LOSS_SCALE <= min_loss_scale); APPLIED = 0          (T, POW1, POW2, SCALARS keep their values)
 *     else:            if clip_norm > 0 && nv > clip_norm: c *= clip_norm / (nv + 1e-6)
 *                      T += 1; POW1 *= beta1; POW2 *= beta2; bias1 = 1 - POW1; sqrt_bias2 = sqrt(1 - POW2)
 *                      SCALARS from (c, LR, beta1, beta2, eps, LR * weight_decay, bias1, sqrt_bias2), derived in double and rounded once
 *                      exactly as dsp_fp16_optim_adam_step derives them; APPLIED = 1
 *                      if (ITER - LAST_OVERFLOW_ITER) % scale_window == 0: LOSS_SCALE *= scale_factor
 *                      ITER += 1
 *     LOSS_SCALE_F32 = (float)LOSS_SCALE
 *   Every operation is an IEEE double multiply, add, divide or square root in this order, compiled with floating-point contraction off (no
 *   fma), so the same lines in host doubles give every slot bit for bit; the bias corrections are running products, not pow().  The constants
 *   of the optimizer's life are arguments: clip_norm <= 0 means no clipping.  Plain stores, no atomics.
 *   DSP_EINVAL: S or state null or off an 8-byte boundary, a beta outside [0, 1), scale_factor <= 1, scale_window < 1. */
int dsp_fp16_optim_scale_step(const double* S, void* state, double beta1, double beta2, double eps, double weight_decay, double clip_norm,
                              double scale_factor, int64_t scale_window, double min_loss_scale, dsp_stream_t stream);

/* dsp_fp16_optim_adam_step with its scalars read from the state: the same kernel code, per element the same bits for equal scalars.  With
 * APPLIED == 0 every workgroup returns before its first store: master, moments and parameters keep their values.
 *   N == 0 or n_items == 0: DSP_OK, nothing launched, no pointer looked at.  DSP_EINVAL: as dsp_fp16_optim_adam_step (tables, flat arrays,
 *   dtype, chunk), and a state that is null or off an 8-byte boundary. */
int dsp_fp16_optim_adam_step_state(const void* const* grads, void* const* params16, int dtype, const int64_t* offsets, int N,
                                   const int64_t* items, int64_t n_items, int chunk, float* master, float* exp_avg, float* exp_avg_sq,
                                   const void* state, dsp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
