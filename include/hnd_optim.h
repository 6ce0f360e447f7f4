/*
 * hnd_optim.h -- the optimizer kinds of libhnd_hip.so beyond hnd_adam_step_flat / hnd_sgd_step_flat (hnd_hip.h):
 * torch.optim.Adam with weight_decay and / or amsgrad, torch.optim.Adagrad and torch.optim.RMSprop, which the reference
 * reaches through func_util.get_optimizer(model, type, params) (src/myutils/pytorch/func_util.py, called at
 * src/mimic_runner.py:67-68) for any `optimizer: {type: ..., params: ...}` section of a config.
 *
 * A header of its own with a version of its own: hnd_hip.h and HND_ABI_VERSION are unchanged by it.  The conventions are
 * those of hnd_hip.h: device pointers into caller-owned buffers, `stream` is a hipStream_t passed as void*, 0 on success
 * and a negative hnd_status otherwise, hnd_last_error_string() explains.
 *
 * One launch per call over `numel` fp32 elements; every element of every buffer is read at most once and stored at most
 * once, in a fixed order (bit-reproducible).  The arithmetic is that of torch's single-tensor paths
 * (torch/optim/adam.py, adagrad.py, rmsprop.py: _single_tensor_*, maximize = False, not capturable, not differentiable),
 * in fp32 per element; lerp(a, b, w) is torch's: a + w (b - a) for w < 0.5, else b - (b - a)(1 - w).  Where a product is
 * added to a sum (g, the moments, the final p -= ...) the two are one fused multiply-add, written out in the kernel, so an
 * element gets the same bits whichever access path (16-byte body, scalar tail, unaligned build) reaches it.
 *
 *   every kind    g = grad * grad_scale + weight_decay * p
 *
 *   HND_OPTIM_ADAM      state0 = exp_avg (m), state1 = exp_avg_sq (v), state2 = max_exp_avg_sq (vmax; only with amsgrad)
 *     m = lerp(m, g, 1 - beta1)
 *     v = beta2 * v + (1 - beta2) * g * g
 *     amsgrad:  vmax = max(vmax, v);  u = vmax         else  u = v
 *     denom = sqrt(u) / sqrt(1 - beta2^step) + eps
 *     p -= lr / (1 - beta1^step) * (m / denom)
 *
 *   HND_OPTIM_ADAGRAD   state0 = sum
 *     clr = lr / (1 + (step - 1) * lr_decay)
 *     sum += g * g
 *     p -= clr * (g / (sqrt(sum) + eps))
 *
 *   HND_OPTIM_RMSPROP   state0 = square_avg (sq), state1 = momentum_buffer (buf; only with momentum > 0),
 *                       state2 = grad_avg (ga; only with centered); alpha is passed in beta2
 *     sq = alpha * sq + (1 - alpha) * g * g
 *     centered:  ga = lerp(ga, g, 1 - alpha);  avg = sqrt(sq - ga * ga) + eps      else  avg = sqrt(sq) + eps
 *     momentum > 0:  buf = momentum * buf + g / avg;  p -= lr * buf                else  p -= lr * (g / avg)
 *
 * The scalars that depend on the step or on a difference of hyper-parameters (1 - beta, 1 - beta^step and its root,
 * lr / (1 - beta1^step), clr) are computed on the host in double and rounded to fp32 once, as hnd_adam_step_flat does.
 *
 * Pointers need 4-byte alignment only (the per-tensor host path hands in views at any element offset).  When param, grad
 * and every state buffer the kind uses are 16-byte aligned the launch moves 16 bytes per lane and finishes numel % 4 with
 * scalar accesses; otherwise every access is scalar.  Nothing outside [0, numel) of any buffer is read or written.
 * A state pointer the kind / flags do not use is ignored and may be NULL.
 *
 * Refused with HND_ERR_INVALID before any launch: a NULL descriptor, param or grad; a NULL state pointer the kind / flags
 * use; numel <= 0; step < 1; an unknown kind; any hyper-parameter or grad_scale that is NaN or infinite; lr < 0, eps < 0,
 * weight_decay < 0, momentum < 0, lr_decay < 0; ADAM with beta1 or beta2 outside [0, 1); RMSPROP with alpha (beta2) < 0
 * -- torch's own constructor checks.
 */
#ifndef HND_OPTIM_H
#define HND_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HND_OPTIM_ABI 1

typedef enum hnd_optim_kind {
  HND_OPTIM_ADAM = 0,
  HND_OPTIM_ADAGRAD = 1,
  HND_OPTIM_RMSPROP = 2
} hnd_optim_kind;

typedef struct hnd_optim_desc {
  float* param;
  const float* grad;
  float* state0;          /* ADAM exp_avg,        ADAGRAD sum,  RMSPROP square_avg                        */
  float* state1;          /* ADAM exp_avg_sq,                   RMSPROP momentum_buffer (momentum > 0)    */
  float* state2;          /* ADAM max_exp_avg_sq (amsgrad),     RMSPROP grad_avg (centered)               */
  int64_t numel;
  int64_t step;           /* 1-based count of the step being taken */
  double grad_scale;      /* factor on grad (1 / world size of a summed all-reduce; 1 otherwise) */
  double lr, weight_decay, eps;
  double beta1;           /* ADAM */
  double beta2;           /* ADAM beta2, RMSPROP alpha */
  double momentum;        /* RMSPROP */
  double lr_decay;        /* ADAGRAD */
  int32_t kind;           /* hnd_optim_kind */
  int32_t amsgrad;        /* ADAM */
  int32_t centered;       /* RMSPROP */
  int32_t reserved;       /* 0 */
} hnd_optim_desc;

int hnd_optim_abi(void);   /* HND_OPTIM_ABI */
int hnd_optim_step_flat(const hnd_optim_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HND_OPTIM_H */
