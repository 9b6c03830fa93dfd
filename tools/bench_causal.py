'''
What the causal encoder's block kernel and a stream session cost, measured in ONE process on one box with INTERLEAVED
blocks; prints one JSON line and writes it to profiles/causal_bench.json.  Every row carries the per-block figures,
their median and the block-to-block spread (max - min): a difference inside the spread counts as equal.

  (a) danet_causal_lstm_block through the C entry point at L = 4, H = 600, D0 = 257, B = 1 for Tb in {1, 4, 16, 64}:
      us per block (Tb + L launches) and per frame, --reps back-to-back calls between two events per block.  The
      yardstick of the same run: the whole-utterance `lstm-causal` encoder forward (ops.CausalRnnEncoderFn on the
      core's recurrent kernels) at T = 1251, B = 1, per frame.
  (b) SeparationStream.push end to end (front-end, centring, LSTM block, centring, projection, online scan, separator,
      phase re-attachment, host code included; a host clock around calls that end in a device synchronise) at the cfg-5
      shape (FFT 512 / 128, 16 kHz, E = 20, C = 2, 4 x 600) for blocks of 1, 8 and 32 frames past the hold, and the
      real-time factor = time per block / (n * FFT_STRIDE / SMPRATE).

The one bar: the real-time factor at n = 1 is below 1 (a frame is 8 ms of signal).  Everything else is reported.

    python tools/bench_causal.py [--rounds 5] [--reps 20] [--out FILE]
'''
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L, H, D0, E, C = 4, 600, 257, 20, 2
FFT_SIZE, FFT_STRIDE, SMPRATE = 512, 128, 16000
BLOCK_TB = (1, 4, 16, 64)
PUSH_N = (1, 8, 32)
WHOLE_T = 1251
HP = dict(BATCH_SIZE=1, MAX_N_SIGNAL=C, FFT_SIZE=FFT_SIZE, FFT_STRIDE=FFT_STRIDE, SMPRATE=SMPRATE, EMBED_SIZE=E,
          NUM_ANCHOR=6, NUM_LSTM_LAYERS=L, ENCODER_TYPE='lstm-causal', TRAIN_ESTIMATOR_METHOD='truth-weighted',
          INFER_ESTIMATOR_METHOD='online', SEPARATOR_TYPE='dot-softmax-orig')


def _summary(blocks):
    import numpy as np
    return dict(blocks=[round(float(v), 3) for v in blocks], median=round(float(np.median(blocks)), 3),
                spread=round(float(max(blocks) - min(blocks)), 3))


def _timed_launches(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def block_rows(model, rounds, reps):
    '''(a): {Tb: us per block}, the whole-utterance forward, and the per-frame figures'''
    import torch
    from danet_amd import _lib, ops
    stream = model.open_stream(1)
    lib, st, p = _lib.load_causal(), _lib.stream(), _lib.ptr
    wp = (_lib.c_p * L)(*[p(W) for W in stream.Ws])
    bp = (_lib.c_p * L)(*[p(b) for b in stream.bs])
    gen = torch.Generator().manual_seed(0)
    fns = {}
    for Tb in BLOCK_TB:
        x = torch.randn(Tb, 1, 260, generator=gen).cuda()
        y = torch.empty(Tb, 1, H, device='cuda')
        ws = torch.empty(ops.causal_lstm_ws_bytes(L, 1, Tb, H) // 4, device='cuda')

        def block(Tb=Tb, x=x, y=y, ws=ws):                  # the state keeps running: every call is Tb more frames
            assert lib.danet_causal_lstm_block(st, L, 1, Tb, D0, H, p(x), 260, wp, bp, p(stream.h), p(stream.c), p(y), H,
                                               p(ws), ws.numel() * 4) == 0
        fns['block_Tb%d' % Tb] = block
    xw = torch.randn(1, WHOLE_T, D0, generator=gen).cuda()
    params = [t for pair in zip(stream.Ws, stream.bs) for t in pair] + [stream.Wout]

    def whole():
        with torch.no_grad():
            ops.CausalRnnEncoderFn.apply(xw, H, L, *params)
    fns['whole_utterance_forward_T%d' % WHOLE_T] = whole
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(stream.h).all())
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps if k.startswith('block') else max(1, reps // 10)))
    r = dict(shape=dict(L=L, H=H, D0=D0, B=1), unit='us per call, back to back', weight_bytes=sum(W.numel() * 4 for W in stream.Ws))
    r.update({k: _summary(v) for k, v in t.items()})
    r['us_per_frame'] = {k: round(r[k]['median'] / (WHOLE_T if k.startswith('whole') else int(k.split('Tb')[1])), 3) for k in fns}
    r['launches_per_block'] = {'block_Tb%d' % Tb: Tb + L for Tb in BLOCK_TB}
    print('LSTM block us per frame: %s' % ', '.join('%s %.2f' % kv for kv in r['us_per_frame'].items()), file=sys.stderr)
    return r


def push_rows(model, rounds, reps):
    '''(b): {n: ms per push of n frames past the hold} and the real-time factors'''
    import torch
    T0 = model.online[0]
    gen = torch.Generator().manual_seed(1)
    F = FFT_SIZE // 2 + 1
    mix = torch.view_as_complex(torch.randn(1, T0 + 64, F, 2, generator=gen)).cuda() * 3
    streams = {n: model.open_stream(1) for n in PUSH_N}
    for n, s in streams.items():
        assert s.push(mix[:, :T0]).shape[2] == T0               # past the hold
        for _ in range(3):
            assert s.push(mix[:, T0:T0 + n]).shape[2] == n
    torch.cuda.synchronize()
    t = {n: [] for n in PUSH_N}
    for _ in range(rounds):
        for n, s in streams.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                out = s.push(mix[:, T0:T0 + n])
            torch.cuda.synchronize()
            t[n].append((time.perf_counter() - t0) * 1e3 / reps)
            assert bool(torch.isfinite(torch.view_as_real(out)).all())
    r = dict(shape=dict(FFT_SIZE=FFT_SIZE, FFT_STRIDE=FFT_STRIDE, SMPRATE=SMPRATE, E=E, C=C, L=L, H=H, B=1, T0=T0),
             unit='ms per push, host clock around %d pushes that end in a device synchronise' % reps)
    for n in PUSH_N:
        r['push_n%d' % n] = _summary(t[n])
    r['real_time_factor'] = {'push_n%d' % n: round(r['push_n%d' % n]['median'] * 1e-3 / (n * FFT_STRIDE / SMPRATE), 4)
                             for n in PUSH_N}
    print('push ms: %s; real-time factor: %s' % (', '.join('n=%d %.3f' % (n, r['push_n%d' % n]['median']) for n in PUSH_N),
                                                 r['real_time_factor']), file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_causal.py measures on the GPU'
    torch.cuda.set_device(0)
    from danet_amd.hparams import hparams
    from danet_amd.model import Model
    hparams.load(HP)
    hparams.digest()
    model = Model('causal_bench', device='cuda:0', seed=1).build()
    res = dict(workload='causal encoder: danet_causal_lstm_block per block and per frame next to the whole-utterance '
                        'lstm-causal forward, and SeparationStream.push end to end with its real-time factor; '
                        'interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, device=torch.cuda.get_device_name(0))
    res['lstm_block'] = block_rows(model, args.rounds, args.reps)
    res['push'] = push_rows(model, args.rounds, args.reps)
    res['bar_real_time_factor_n1_below_1'] = bool(res['push']['real_time_factor']['push_n1'] < 1)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'causal_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    assert res['bar_real_time_factor_n1_below_1'], res['push']['real_time_factor']


if __name__ == '__main__':
    main()
