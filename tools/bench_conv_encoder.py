'''
Times the `conv-bilstm-v1` encoder at the cfg-2 shape (B = 32, T = 128, FFT 256 / stride 64,
C = 2, E = 20, anchor estimator, softmax separator) and prints ONE JSON line:

  * whole train steps (forward + backward + Adam through Model.train_step): warm-up, then
    --steps steps closed by one device synchronise -> ms/step and mixture-s/s
    (mixture-seconds per step = B * T * FFT_STRIDE / SMPRATE = 32.768);
  * every conv layer's forward, data-gradient and weight-gradient launches on their own, with
    TFLOP/s from the algorithmic FLOPs 2 * B * T * F * Cin * Cout * k^2 (pre-pool output grid);
  * for comparison, torch's fp32 conv2d (MIOpen) at the same shapes in contiguous NCHW: forward,
    torch.nn.grad.conv2d_input and conv2d_weight.  Measured here only; the encoder never calls it.

    python tools/bench_conv_encoder.py [--steps 100] [--warmup 10] [--reps 20]
'''
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def layer_times(B, T, nfft, alpha, reps):
    import torch
    import torch.nn.functional as Fn
    from danet_amd import ops
    out = []
    g = torch.Generator(device='cuda').manual_seed(0)
    for l, d in enumerate(ops.conv_encoder_descs(B, T, nfft, alpha)):
        xs, ys = tuple(d.x_stride), tuple(d.y_stride)
        if d.pool:
            yshape = (d.B, d.Cout, d.T // 2, d.F // 2)
        elif d.d2s:
            yshape = (d.B, d.Cout // 4, 2 * d.T, 2 * d.F)
        else:
            yshape = (d.B, d.Cout, d.T, d.F)
        span = lambda shape, st: sum((n - 1) * s for n, s in zip(shape, st)) + 1
        x = torch.randn(span((d.B, d.Cin, d.T, d.F), xs), device='cuda', generator=g)
        y = torch.empty(span(yshape, ys), device='cuda')
        dy = torch.randn(span(yshape, ys), device='cuda', generator=g)
        dx = torch.empty_like(x)
        w = torch.randn(d.k, d.k, d.Cin, d.Cout, device='cuda', generator=g) * 0.1
        b = torch.zeros(d.Cout, device='cuda')
        dw, db = torch.empty_like(w), torch.empty_like(b)
        am = torch.empty(d.B, d.Cout, d.T // 2, d.F // 2, dtype=torch.uint8, device='cuda') if d.pool else None
        flop = 2.0 * d.B * d.T * d.F * d.Cin * d.Cout * d.k * d.k
        t_f = _time(lambda: ops.conv_fwd(d, x, w, b, y, am), reps)
        t_d = _time(lambda: ops.conv_bwd_data(d, dy, y, am, w, dx), reps) if l > 0 else None
        t_w = _time(lambda: ops.conv_bwd_weight(d, x, dy, y, am, dw, db), reps)
        # torch / MIOpen fp32 at the same shape, contiguous NCHW, no pool / depth-to-space
        xt = torch.randn(d.B, d.Cin, d.T, d.F, device='cuda', generator=g)
        wt = torch.randn(d.Cout, d.Cin, d.k, d.k, device='cuda', generator=g) * 0.1
        bt = torch.zeros(d.Cout, device='cuda')
        gt = torch.randn(d.B, d.Cout, d.T, d.F, device='cuda', generator=g)
        pad = d.k // 2
        m_f = _time(lambda: Fn.conv2d(xt, wt, bt, padding=pad), reps)
        m_d = _time(lambda: torch.nn.grad.conv2d_input(xt.shape, wt, gt, padding=pad), reps) if l > 0 else None
        m_w = _time(lambda: torch.nn.grad.conv2d_weight(xt, wt.shape, gt, padding=pad), reps)
        tf = lambda ms: None if ms is None else round(flop / ms / 1e9, 2)
        r3 = lambda v: None if v is None else round(v, 4)
        out.append(dict(layer=('conv2d' if l == 0 else 'conv2d_%d' % l), gflop=round(flop / 1e9, 3),
                        fwd_ms=r3(t_f), dgrad_ms=r3(t_d), wgrad_ms=r3(t_w),
                        fwd_tflops=tf(t_f), dgrad_tflops=tf(t_d), wgrad_tflops=tf(t_w),
                        miopen_fwd_ms=r3(m_f), miopen_dgrad_ms=r3(m_d), miopen_wgrad_ms=r3(m_w)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.load_package()
    from danet_amd.hparams import hparams
    from danet_amd.model import Model
    from danet_amd import ops
    torch.cuda.set_device(0)
    hp = dict(BATCH_SIZE=32, MAX_N_SIGNAL=2, FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000, EMBED_SIZE=20,
              NUM_ANCHOR=6, ENCODER_TYPE='conv-bilstm-v1', TRAIN_ESTIMATOR_METHOD='anchor',
              INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig')
    hparams.reset()
    hparams.load(hp)
    hparams.digest()
    B, T, F, C = 32, 128, hparams.FEATURE_SIZE, 2
    model = Model('bench_conv', device='cuda:0').build()
    rng = np.random.RandomState(0)
    src = torch.as_tensor(((rng.randn(B, C, T, F) + 1j * rng.randn(B, C, T, F)) * 4).astype(np.complex64)).cuda()
    for _ in range(args.warmup):
        model.train_step(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = model.train_step(src)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    loss = float(out['loss'])
    assert ops.lstm_status_ok() and np.isfinite(loss)
    layers = layer_times(B, T, 256, float(hparams.RELU_LEAKAGE), args.reps)
    tot = sum(v for r in layers for v in (r['fwd_ms'], r['dgrad_ms'], r['wgrad_ms']) if v is not None)
    mio = sum(v for r in layers for v in (r['miopen_fwd_ms'], r['miopen_dgrad_ms'], r['miopen_wgrad_ms'])
              if v is not None)
    mix_s = B * T * hparams.FFT_STRIDE / hparams.SMPRATE
    print(json.dumps(dict(workload='conv-bilstm-v1 cfg2 train step', steps=args.steps, ms_per_step=round(ms, 3),
                          mixture_s_per_s=round(mix_s / ms * 1e3, 1), loss=loss,
                          conv_fwd_bwd_ms=round(tot, 3), miopen_conv_fwd_bwd_ms=round(mio, 3),
                          layers=layers)))


if __name__ == '__main__':
    main()
