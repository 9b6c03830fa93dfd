'''
What the waveform metric of valid / test (EVAL_SI_SDR) costs, measured in ONE process on one box with
INTERLEAVED blocks; prints one JSON line and writes it to profiles/metric_bench.json.  Every row carries the
per-block figures, their median and the block-to-block spread (max - min): a difference inside the spread counts
as equal.

  (a) the three entry points at the cfg-2 validation shape (B = 32, C = 2, T = 128, N = 256, S = 64): --reps
      back-to-back calls through the C entry point between two events per block, us per call -- each alone and
      the chain of the three -- next to the launch floor of the same run (danet_metric_si_sdr on one
      utterance of one source);
  (b) Model.valid_step at cfg 2 with the key on against the key off: two models of the same seed, --reps
      back-to-back steps between two events per block, us per step.

No bar: the figures are reported.

    python tools/bench_metric.py [--rounds 7] [--reps 50] [--step-reps 20] [--out FILE]
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
    hparams.reset()
    hparams.load(dict(FFT_SIZE=N, FFT_STRIDE=S))
    hparams.digest()
    a, b, per_utt, perm = ops.si_sdr(src, est)                   # (maps the library, sizes the scratch)
    lib, st = _lib.load_metric(), _lib.stream()
    _, wav, G, pu, mean2, pi = ops._wave_workspace('metric', ops._metric_ws, 2 * C, 2, B, C, T, N, S, src.device)
    w = ops._metric_window(src.device)
    one_G = torch.eye(2, dtype=torch.float64, device='cuda')[None].contiguous()
    one_out = torch.zeros(8, dtype=torch.float64, device='cuda')
    one_perm = torch.zeros(1, dtype=torch.int32, device='cuda')
    rs, re_ = torch.view_as_real(src).data_ptr(), torch.view_as_real(est).data_ptr()

    def synth():
        assert lib.danet_metric_synth(st, B, C, T, N, S, rs, re_, w.data_ptr(), wav.data_ptr()) == 0

    def gram():
        assert lib.danet_metric_gram(st, B, 2 * C, (T - 1) * S, wav.data_ptr(), G.data_ptr()) == 0

    def final():
        assert lib.danet_metric_si_sdr(st, B, C, G.data_ptr(), pu.data_ptr(), pi.data_ptr(), mean2.data_ptr()) == 0

    def chain():
        synth()
        gram()
        final()

    def floor():
        assert lib.danet_metric_si_sdr(st, 1, 1, one_G.data_ptr(), one_out.data_ptr(), one_perm.data_ptr(),
                                       one_out.data_ptr() + 16) == 0
    fns = dict(synth=synth, gram=gram, si_sdr=final, chain_of_three=chain, launch_floor=floor)
    for _ in range(20):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    assert torch.equal(pu, per_utt) and torch.equal(pi, perm)     # two routes, bit for bit
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    r = dict(shape=dict(B=B, C=C, T=T, N=N, S=S), signals=B * 2 * C, samples_per_signal=(T - 1) * S,
             unit='us per call, back to back, C entry point', si_sdr_db=float(a), si_sdri_db=float(b))
    r.update({k: _summary(v) for k, v in t.items()})
    print('entry points: synth %.1f, gram %.1f, si_sdr %.1f, chain %.1f us; launch floor %.1f us'
          % tuple(r[k]['median'] for k in fns), file=sys.stderr)
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
    models = {}
    for tag, key in (('key_off', None), ('key_on', True)):
        hparams.reset()
        hparams.load(dict(base, EVAL_SI_SDR=key))
        hparams.digest()
        models[tag] = Model('bench_metric', device='cuda:0', seed=7).build()
    last = {}

    def step(tag):
        def fn():
            last[tag] = models[tag].valid_step(src)
        return fn
    for _ in range(5):
        for tag in models:
            step(tag)()
    torch.cuda.synchronize()
    assert float(last['key_off']['loss']) == float(last['key_on']['loss'])
    t = {tag: [] for tag in models}
    for _ in range(rounds):
        for tag in models:
            t[tag].append(_timed_launches(step(tag), reps))
    for m in models.values():
        m.check_status()
    r = dict(config='cfg2', unit='us per valid_step, back to back', key_off=_summary(t['key_off']),
             key_on=_summary(t['key_on']), si_sdr_db=float(last['key_on']['SI-SDR']),
             si_sdri_db=float(last['key_on']['SI-SDRi']))
    r['added_us_per_step'] = round(r['key_on']['median'] - r['key_off']['median'], 2)
    print('valid_step: key off %.1f us (spread %.1f), key on %.1f us (spread %.1f): +%.1f us'
          % (r['key_off']['median'], r['key_off']['spread'], r['key_on']['median'], r['key_on']['spread'],
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
    assert torch.cuda.is_available(), 'bench_metric.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='waveform SI-SDR of valid / test: synthesis, Gram, finalize; interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, step_reps=args.step_reps, device=torch.cuda.get_device_name(0))
    res['a_entry_points_cfg2'] = entry_points_row(args.rounds, args.reps)
    res['b_valid_step_cfg2'] = valid_step_row(args.rounds, args.step_reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'metric_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
