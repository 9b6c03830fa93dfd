'''
What the waveform training loss (TRAIN_LOSS = "si-sdr") costs, measured in ONE process on one box with
INTERLEAVED blocks; prints one JSON line and writes it to profiles/wavloss_bench.json.  Every row carries the
per-block figures, their median and the block-to-block spread (max - min): a difference inside the spread counts
as equal.

  (a) the entry points at the cfg-2 shape (B = 32, C = 2, T = 128, N = 256, S = 64): --reps back-to-back calls
      through the C entry point between two events per block, us per call -- danet_wavloss_fwd, danet_wavloss_bwd
      in both output forms, and the forward chain (danet_metric_synth, danet_metric_gram, danet_wavloss_fwd) --
      next to danet_metric_synth and the launch floor of the same run (danet_wavloss_fwd on one utterance of one
      source);
  (b) Model.train_step at cfg 2 with the key "si-sdr" against the key null: two models of the same seed, --reps
      back-to-back steps between two events per block, us per step.

No bar: the figures are reported.

    python tools/bench_wavloss.py [--rounds 7] [--reps 50] [--step-reps 20] [--out FILE]
'''
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


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


def entry_points_row(rounds, reps, B=32, C=2, T=128, N=256, S=64):
    import numpy as np
    import torch
    from danet_amd import _lib, ops
    from danet_amd.hparams import hparams
    rng = np.random.RandomState(0)
    F = N // 2 + 1
    src = torch.from_numpy((rng.randn(B, C, T, F) + 1j * rng.randn(B, C, T, F)).astype(np.complex64)).cuda()
    est = torch.from_numpy((rng.randn(B, C, T, F) + 1j * rng.randn(B, C, T, F)).astype(np.complex64)).cuda() + src
    ang = torch.from_numpy(rng.uniform(-np.pi, np.pi, (B, T, F)).astype(np.float32)).cuda()
    phasor = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).contiguous()
    hparams.reset()
    hparams.load(dict(FFT_SIZE=N, FFT_STRIDE=S))
    hparams.digest()
    w = ops._metric_window(src.device)
    wav = ops.metric_synth(src, est, S, w)
    G = ops.metric_gram(wav)
    loss64, loss32, per_utt, perm, pair, coef = ops.wavloss_fwd(G)          # (maps the library)
    dX = ops.wavloss_bwd(wav, pair, coef, N, S, window=w)
    dsep = ops.wavloss_bwd(wav, pair, coef, N, S, window=w, phasor=phasor)
    mlib, lib, st = _lib.load_metric(), _lib.load_wavloss(), _lib.stream()
    one_G = torch.eye(2, dtype=torch.float64, device='cuda')[None].contiguous()
    one_f64 = torch.zeros(8, dtype=torch.float64, device='cuda')
    one_i32 = torch.zeros(8, dtype=torch.int32, device='cuda')
    one_f32 = torch.zeros(2, dtype=torch.float32, device='cuda')
    rs, re_ = torch.view_as_real(src).data_ptr(), torch.view_as_real(est).data_ptr()

    def synth():
        assert mlib.danet_metric_synth(st, B, C, T, N, S, rs, re_, w.data_ptr(), wav.data_ptr()) == 0

    def gram():
        assert mlib.danet_metric_gram(st, B, 2 * C, (T - 1) * S, wav.data_ptr(), G.data_ptr()) == 0

    def fwd():
        assert lib.danet_wavloss_fwd(st, B, C, G.data_ptr(), loss64.data_ptr(), loss32.data_ptr(), per_utt.data_ptr(),
                                     perm.data_ptr(), pair.data_ptr(), coef.data_ptr()) == 0

    def bwd_complex():
        assert lib.danet_wavloss_bwd(st, B, C, T, N, S, wav.data_ptr(), pair.data_ptr(), coef.data_ptr(), w.data_ptr(),
                                     None, None, torch.view_as_real(dX).data_ptr()) == 0

    def bwd_real():
        assert lib.danet_wavloss_bwd(st, B, C, T, N, S, wav.data_ptr(), pair.data_ptr(), coef.data_ptr(), w.data_ptr(),
                                     None, phasor.data_ptr(), dsep.data_ptr()) == 0

    def chain():
        synth()
        gram()
        fwd()

    def floor():
        assert lib.danet_wavloss_fwd(st, 1, 1, one_G.data_ptr(), one_f64.data_ptr(), one_f32.data_ptr(),
                                     one_f64.data_ptr() + 8, one_i32.data_ptr(), one_i32.data_ptr() + 4,
                                     one_f64.data_ptr() + 16) == 0
    fns = dict(wavloss_fwd=fwd, wavloss_bwd_complex=bwd_complex, wavloss_bwd_real=bwd_real, forward_chain=chain,
               metric_synth=synth, launch_floor=floor)
    keep = [v.clone() for v in (loss64, pair, coef, dX, dsep)]
    for _ in range(20):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    for a, b in zip(keep, (loss64, pair, coef, dX, dsep)):            # two routes, bit for bit
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b)
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    r = dict(shape=dict(B=B, C=C, T=T, N=N, S=S), estimates=B * C, samples_per_signal=(T - 1) * S,
             tile_frames=ops.wavloss_tile_frames(N), unit='us per call, back to back, C entry point',
             loss_db=float(loss64))
    r.update({k: _summary(v) for k, v in t.items()})
    print('entry points: fwd %.1f, bwd complex %.1f, bwd real %.1f, forward chain %.1f, metric_synth %.1f us; launch '
          'floor %.1f us' % tuple(r[k]['median'] for k in fns), file=sys.stderr)
    return r


def train_step_row(rounds, reps):
    import numpy as np
    import torch
    import bench
    from danet_amd.hparams import hparams
    from danet_amd.model import Model
    cfg = bench.CONFIGS['cfg2']
    base = dict(cfg['hp'], BATCH_SIZE=cfg['batch'], NUM_LSTM_LAYERS=cfg['layers'], LSTM_HDIM=cfg['hdim'],
                ENCODER_TYPE='bilstm-orig', OPTIMIZER_TYPE='adam')
    rng = np.random.RandomState(1)
    shape = (cfg['batch'], cfg['hp']['MAX_N_SIGNAL'], cfg['frames'], cfg['hp']['FFT_SIZE'] // 2 + 1)
    src = torch.from_numpy(((rng.randn(*shape) + 1j * rng.randn(*shape)) * 3).astype(np.complex64)).cuda()
    models = {}
    for tag, key in (('key_null', None), ('key_si_sdr', 'si-sdr')):
        hparams.reset()
        hparams.load(dict(base, TRAIN_LOSS=key))
        hparams.digest()
        models[tag] = Model('bench_wavloss', device='cuda:0', seed=7).build()
    last = {}

    def step(tag):
        def fn():
            last[tag] = models[tag].train_step(src)
        return fn
    for _ in range(5):
        for tag in models:
            step(tag)()
    torch.cuda.synchronize()
    t = {tag: [] for tag in models}
    for _ in range(rounds):
        for tag in models:
            t[tag].append(_timed_launches(step(tag), reps))
    for m in models.values():
        m.check_status()
    r = dict(config='cfg2', unit='us per train_step, back to back', key_null=_summary(t['key_null']),
             key_si_sdr=_summary(t['key_si_sdr']), loss_mse=float(last['key_null']['loss']),
             loss_db=float(last['key_si_sdr']['loss']))
    r['added_us_per_step'] = round(r['key_si_sdr']['median'] - r['key_null']['median'], 2)
    print('train_step: key null %.1f us (spread %.1f), key "si-sdr" %.1f us (spread %.1f): +%.1f us'
          % (r['key_null']['median'], r['key_null']['spread'], r['key_si_sdr']['median'], r['key_si_sdr']['spread'],
             r['added_us_per_step']), file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--step-reps', type=int, default=20)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_wavloss.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='waveform training loss: finalize, adjoint of the synthesis, train step; interleaved blocks in '
                        'one process',
               rounds=args.rounds, reps=args.reps, step_reps=args.step_reps, device=torch.cuda.get_device_name(0))
    res['a_entry_points_cfg2'] = entry_points_row(args.rounds, args.reps)
    res['b_train_step_cfg2'] = train_step_row(args.rounds, args.step_reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'wavloss_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
