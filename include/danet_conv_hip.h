/*
 * libdanet_conv_hip.so -- C ABI of the 2-D convolution operators of the
 * `conv-bilstm-v1` encoder (reference app/modules.py:263-379), gfx950 only.
 *
 * An optional extension library beside libdanet_hip.so: the core ABI stays as it
 * is.  Same conventions as include/danet_hip.h: caller-owned DEVICE pointers,
 * fp32, `stream` a hipStream_t passed as void*, 0 = DANET_CONV_OK and negative =
 * error with a thread-local message in danet_conv_last_error(), asynchronous
 * launches, no process environment read, no allocation.
 *
 * The operator (tf.layers.conv2d, data_format='channels_first', padding='same'):
 *     z[b][co][t][f] = bias[co] + sum_{ci,i,j} x[b][ci][t+i-k/2][f+j-k/2] * w[i][j][ci][co]
 *     y = max(alpha * z, z)                                    (leaky ReLU, ops.relu)
 * stride 1, zero padding, k in {3, 5}; `w` in TF's [k][k][Cin][Cout] order.
 * Every tensor is addressed through (b, c, t, f) element strides, so a layer reads and writes
 * the layouts its neighbours use (the LSTM's time-major rows, the dense layer's rows) with no
 * permute copies.  Optional on the output side, one or the other:
 *   pool = 1: 2x2 max-pool, stride 2, 'valid' (Tp = T/2, Fp = F/2 rounded down); `y` holds the
 *             pooled [B][Cout][Tp][Fp] (at y_stride) and `argmax` (uint8, dense [B][Cout][Tp][Fp])
 *             the window position of the first maximum in row-major order (0..3 = 2*dt + df).
 *             A NaN reaches the pooled output only when it is the first element of its window.
 *   d2s = 1:  depth-to-space by 2: y_stride addresses a [B][Cout/4][2T][2F] tensor and
 *             out[c][2t+a][2f+b] = z[4c+2a+b][t][f] (Cout % 4 == 0).
 * Products are exact fp32 (v_mfma_f32_16x16x4_f32) with fp32 accumulation.
 */
#ifndef DANET_CONV_HIP_H
#define DANET_CONV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden and linked against csrc/conv/exports.map: exactly the entry points
 * declared between this push and the pop are exported.                                         */
#pragma GCC visibility push(default)

#define DANET_CONV_ABI_VERSION 1

#define DANET_CONV_OK 0
#define DANET_CONV_ERR_ARG (-1)        /* bad shape / null pointer          */
#define DANET_CONV_ERR_LAUNCH (-2)     /* hipLaunch failure                 */
#define DANET_CONV_ERR_WORKSPACE (-4)  /* ws too small                      */

/* One convolution layer.  Bounds: B, T, F >= 1; 1 <= Cin, Cout <= 64; k in {3, 5};
 * 0 <= alpha < 1; pool needs T, F >= 2; d2s needs Cout % 4 == 0; not both.
 * x_stride: (b, c, t, f) strides of the layer input [B][Cin][T][F] (and of dx);
 * y_stride: strides of the stored output (pooled / depth-to-space as above, and of dy). */
typedef struct {
  int B, Cin, Cout, T, F, k;
  int pool, d2s;
  float alpha;
  int64_t x_stride[4];
  int64_t y_stride[4];
} danet_conv_desc_t;

int danet_conv_abi_version(void);
const char* danet_conv_last_error(void);

/* Scratch sizes: ONE query.  Returns the bytes `ws` needs for `op` on layer `d`, or (size_t)-1
 * for a bad op or descriptor (danet_conv_last_error says which).                            */
enum {
  DANET_CONV_WS_BWD_WEIGHT = 0,   /* danet_conv_bwd_weight: fp32 partial slabs */
  DANET_CONV_WS_COUNT
};
size_t danet_conv_workspace_bytes(int op, const danet_conv_desc_t* d);

/* y = lrelu(conv(x, w) + bias) [-> pool | depth-to-space].  `argmax` is required with pool and
 * ignored otherwise.                                                                        */
int danet_conv_fwd(void* stream, const danet_conv_desc_t* d, const float* x, const float* w,
                   const float* bias, float* y, uint8_t* argmax);

/* dx = full correlation of g with the flipped w, g = dy * (y > 0 ? 1 : alpha) at the
 * pre-pool positions; with pool, dy (at y_stride, like y) reaches only the window position
 * `argmax` names and the rows / columns the 'valid' pool drops get zero.  g is formed in the
 * loader and never stored.  dx at x_stride, overwritten.                                    */
int danet_conv_bwd_data(void* stream, const danet_conv_desc_t* d, const float* dy, const float* y,
                        const uint8_t* argmax, const float* w, float* dx);

/* dw [k][k][Cin][Cout] = sum_{b,t,f} x-patch * g, db [Cout] = sum_{b,t,f} g (g as above).
 * Per-slab fp32 partials go to `ws` (danet_conv_workspace_bytes(DANET_CONV_WS_BWD_WEIGHT, d)),
 * then a second pass sums them in a fixed order: no float atomics, bit-identical from run to
 * run.  accumulate = 1: dw += ..., db += ... (else overwritten).                            */
int danet_conv_bwd_weight(void* stream, const danet_conv_desc_t* d, const float* x, const float* dy,
                          const float* y, const uint8_t* argmax, float* dw, float* db, int accumulate,
                          void* ws, size_t ws_bytes);

/* out[i] = a[i] + b[i], i < n (the encoder's residual and the sum of conv_act's two gradients;
 * out may alias a or b).                                                                    */
int danet_conv_add(void* stream, int64_t n, const float* a, const float* b, float* out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DANET_CONV_HIP_H */
