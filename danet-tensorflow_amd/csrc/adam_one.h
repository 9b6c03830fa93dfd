/*
 * One element of the TF1 Adam update behind value clipping, once: adam_clip_kernel (csrc/pointwise.hip, the core
 * library) and gclip_adam_kernel (csrc/gclip) both run it.
 */
#ifndef DANET_ADAM_ONE_H
#define DANET_ADAM_ONE_H

#include <hip/hip_runtime.h>

__device__ __forceinline__ void adam_one(float& th, float& gi, float& mi, float& vi, float lr_t,
                                         float b1, float b2, float eps, float clip, float gscale) {
  float g = gi * gscale;
  if (clip > 0.f) g = (g != g) ? g : fminf(fmaxf(g, -clip), clip);   /* main.py:359-362 */
  mi = b1 * mi + (1.f - b1) * g;
  vi = b2 * vi + (1.f - b2) * g * g;
  th -= lr_t * mi / (sqrtf(vi) + eps);                              /* eps outside the root (TF1) */
}

#endif
