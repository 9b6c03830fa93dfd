'''
What the metric of a noisy valid / test sweep (NOISE_EVAL_DIR with EVAL_SI_SDR) costs beside the clean metric, measured
in ONE process on one box with INTERLEAVED blocks; prints one JSON line and writes it to profiles/neval_bench.json.
Every row carries the per-block figures, their median and the block-to-block spread (max - min): a difference inside
the spread counts as equal.

  (a) at the cfg-2 validation shape (B = 32, C = 2, T = 128, N = 256, S = 64), through the C entry points: --reps
      back-to-back calls between two events per block, us per call -- danet_neval_synth, danet_neval_gram,
      danet_neval_si_sdr each alone and the chain of the three; in the same blocks the chain of the three
      danet_metric_* entry points (the clean metric) and its parts, and the launch floor of the run
      (danet_neval_si_sdr on one utterance of one source).
      BAR: the new chain takes at most 1.25 x the clean chain of the same run -- the ratio of the signals
      synthesised, 5 to 4 -- a difference inside the spread counting as equal; `bar_met` says which, and the
      per-kernel split is in the row either way.
  (b) Model.valid_step at cfg 2 with EVAL_SI_SDR true, with and without a noise component: one model, --step-reps
      back-to-back steps between two events per block, us per step.

    python tools/bench_neval.py [--rounds 7] [--reps 50] [--step-reps 20] [--out FILE]
'''
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

BAR = 1.25


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

    def spectra(*shape):
        return torch.from_numpy((rng.randn(*shape) + 1j * rng.randn(*shape)).astype(np.complex64)).cuda()
    src = spectra(B, C, T, F)
    est = spectra(B, C, T, F) + src
    noise = spectra(B, T, F)
    gain = torch.from_numpy(rng.uniform(0.2, 2.0, size=B).astype(np.float32)).cuda()
    hparams.reset()
    hparams.load(dict(FFT_SIZE=N, FFT_STRIDE=S))
    hparams.digest()
    a, b, c, per_utt, perm = ops.si_sdr_noisy(src, est, noise, gain)     # (maps the library, sizes the scratch)
    ca, cb, cper, cperm = ops.si_sdr(src, est)
    nlib, mlib, st = _lib.load_neval(), _lib.load_metric(), _lib.stream()
    _, wav, G, pu, mean3, pi = ops._wave_workspace('neval', ops._neval_ws, 2 * C + 1, 3, B, C, T, N, S, src.device)
    _, mwav, mG, mpu, mean2, mpi = ops._wave_workspace('metric', ops._metric_ws, 2 * C, 2, B, C, T, N, S, src.device)
    w = ops._metric_window(src.device)
    one_G = torch.eye(3, dtype=torch.float64, device='cuda')[None].contiguous()
    one_out = torch.zeros(8, dtype=torch.float64, device='cuda')
    one_perm = torch.zeros(1, dtype=torch.int32, device='cuda')
    rs, re_, rn = (torch.view_as_real(x).data_ptr() for x in (src, est, noise))
    Ls = (T - 1) * S

    def synth():
        assert nlib.danet_neval_synth(st, B, C, T, N, S, rs, re_, rn, gain.data_ptr(), w.data_ptr(), wav.data_ptr()) == 0

    def gram():
        assert nlib.danet_neval_gram(st, B, 2 * C + 1, Ls, wav.data_ptr(), G.data_ptr()) == 0

    def final():
        assert nlib.danet_neval_si_sdr(st, B, C, G.data_ptr(), pu.data_ptr(), pi.data_ptr(), mean3.data_ptr()) == 0

    def chain():
        synth()
        gram()
        final()

    def msynth():
        assert mlib.danet_metric_synth(st, B, C, T, N, S, rs, re_, w.data_ptr(), mwav.data_ptr()) == 0

    def mgram():
        assert mlib.danet_metric_gram(st, B, 2 * C, Ls, mwav.data_ptr(), mG.data_ptr()) == 0

    def mfinal():
        assert mlib.danet_metric_si_sdr(st, B, C, mG.data_ptr(), mpu.data_ptr(), mpi.data_ptr(), mean2.data_ptr()) == 0

    def mchain():
        msynth()
        mgram()
        mfinal()

    def floor():
        assert nlib.danet_neval_si_sdr(st, 1, 1, one_G.data_ptr(), one_out.data_ptr(), one_perm.data_ptr(),
                                       one_out.data_ptr() + 32) == 0
    fns = dict(neval_synth=synth, neval_gram=gram, neval_si_sdr=final, neval_chain=chain, metric_synth=msynth,
               metric_gram=mgram, metric_si_sdr=mfinal, metric_chain=mchain, launch_floor=floor)
    for _ in range(20):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    assert torch.equal(pu, per_utt) and torch.equal(pi, perm)     # two routes, bit for bit
    assert torch.equal(mpu, cper) and torch.equal(mpu[:, 0], pu[:, 0])
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    r = dict(shape=dict(B=B, C=C, T=T, N=N, S=S), signals=B * (2 * C + 1), signals_clean=B * 2 * C,
             samples_per_signal=Ls, unit='us per call, back to back, C entry point', si_sdr_db=float(a),
             si_sdri_db=float(b), nsnr_db=float(c), si_sdri_clean_db=float(cb))
    r.update({k: _summary(v) for k, v in t.items()})
    new, old = r['neval_chain'], r['metric_chain']
    r['chain_ratio'] = round(new['median'] / old['median'], 4)
    r['bar'] = BAR
    # a difference inside the spread counts as equal: the bar is missed only by more than the larger spread
    r['bar_met'] = bool(new['median'] <= BAR * old['median'] + max(new['spread'], old['spread']))
    print('neval: synth %.1f, gram %.1f, si_sdr %.1f, chain %.1f us; metric: synth %.1f, gram %.1f, si_sdr %.1f, '
          'chain %.1f us; launch floor %.1f us; chain ratio %.3f (bar %.2f: %s)'
          % (tuple(r[k]['median'] for k in fns) + (r['chain_ratio'], BAR, 'met' if r['bar_met'] else 'MISSED')),
          file=sys.stderr)
    return r


def valid_step_row(rounds, reps):
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
    nshape = (shape[0],) + shape[2:]
    noise = torch.from_numpy(((rng.randn(*nshape) + 1j * rng.randn(*nshape)) * 3).astype(np.complex64)).cuda()
    gain = torch.from_numpy(rng.uniform(0.2, 2.0, size=shape[0]).astype(np.float32)).cuda()
    hparams.reset()
    hparams.load(dict(base, EVAL_SI_SDR=True))
    hparams.digest()
    model = Model('bench_neval', device='cuda:0', seed=7).build()
    last = {}

    def clean():
        last['clean'] = model.valid_step(src)

    def noisy():
        last['noisy'] = model.valid_step(src, s_noise=noise, s_noise_gain=gain)
    fns = dict(clean=clean, noisy=noisy)
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {tag: [] for tag in fns}
    for _ in range(rounds):
        for tag, fn in fns.items():
            t[tag].append(_timed_launches(fn, reps))
    model.check_status()
    r = dict(config='cfg2', unit='us per valid_step with EVAL_SI_SDR true, back to back', clean=_summary(t['clean']),
             noisy=_summary(t['noisy']), noisy_metrics={k: float(v) for k, v in last['noisy'].items()},
             clean_metrics={k: float(v) for k, v in last['clean'].items()})
    r['added_us_per_step'] = round(r['noisy']['median'] - r['clean']['median'], 2)
    print('valid_step: clean %.1f us (spread %.1f), noisy %.1f us (spread %.1f): %+.1f us'
          % (r['clean']['median'], r['clean']['spread'], r['noisy']['median'], r['noisy']['spread'],
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
    assert torch.cuda.is_available(), 'bench_neval.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='SI-SDR / SI-SDRi / nSNR of a noisy valid / test sweep beside the clean metric: synthesis, '
                        'Gram, finalize; interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, step_reps=args.step_reps, device=torch.cuda.get_device_name(0))
    res['a_entry_points_cfg2'] = entry_points_row(args.rounds, args.reps)
    res['b_valid_step_cfg2'] = valid_step_row(args.rounds, args.step_reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'neval_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
