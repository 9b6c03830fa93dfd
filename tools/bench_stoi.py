'''
What the intelligibility figures of valid / test (EVAL_STOI) cost, measured in ONE process on one box with INTERLEAVED
blocks; prints one JSON line and writes it to profiles/stoi_bench.json.  Every row carries the per-block figures,
their median and the block-to-block spread (max - min): a difference inside the spread counts as equal.

  (a) the stages at the cfg-2 validation shape (B = 32, C = 2, T = 128, N = 256, S = 64, 8 kHz): --reps back-to-back
      calls through the C entry point between two events per block, us per call, next to the launch floor of the same
      run (danet_stoi_finalize on one utterance of one source).
  (b) the whole device route for the batch (ops.stoi_eval from spectra: synthesis and the five stages) against the
      float64 restatement of tests/stoi_ref.py on the same waveforms on the host with 16 threads.  THE ONE BAR: the
      device route must be faster, otherwise the library has no reason to exist.
  (c) Model.valid_step at cfg 2 with the key on against the key off.

    python tools/bench_stoi.py [--rounds 5] [--reps 20] [--step-reps 5] [--out FILE]
'''
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HOST_THREADS = 16
SMPRATE = 8000


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


def _spectra(B, C, T, seed):
    '''the STFT (N = 256, S = 64) of gated AR(1) references and noisy estimates: frames do get removed'''
    import numpy as np
    import torch
    import stoi_ref as SR
    Ls = (T - 1) * 64 + 256
    win = torch.hann_window(256, periodic=True, dtype=torch.float64)
    wav = np.stack([SR.make_case(C, Ls, seed=seed + b) for b in range(B)]).astype(np.float64)
    X = torch.stft(torch.from_numpy(wav.reshape(B * 2 * C, Ls)), 256, 64, window=win, center=False,
                   return_complex=True).permute(0, 2, 1).reshape(B, 2 * C, T, 129).to(torch.complex64)
    return X[:, :C].contiguous().cuda(), X[:, C:].contiguous().cuda()


def stages_row(rounds, reps, B=32, C=2, T=128, N=256, S=64):
    import ctypes
    import numpy as np
    import torch
    import stoi_ref as SR
    from danet_amd import _lib, ops
    from danet_amd.hparams import hparams
    hparams.reset()
    hparams.load(dict(FFT_SIZE=N, FFT_STRIDE=S, SMPRATE=SMPRATE))
    hparams.digest()
    src, est = _spectra(B, C, T, 0)
    Ls = (T - 1) * S
    wav = ops.metric_synth(src, est, S)
    tabs = ops.stoi_tables(SMPRATE, wav.device)
    U, D = tabs['U'], tabs['D']
    L10, nf = ops.stoi_lengths(Ls, U, D)
    lib, st = _lib.load_stoi(), _lib.stream()
    w = {name: torch.zeros(shape, dtype=dtype, device='cuda') for name, shape, dtype in ops.stoi_parts(B, C, Ls, U, D)}
    p = {k: v.data_ptr() for k, v in w.items()}
    one = {name: torch.zeros(shape, dtype=dtype, device='cuda') for name, shape, dtype in ops.stoi_parts(1, 1, Ls, U, D)}
    q = {k: v.data_ptr() for k, v in one.items()}
    h, win, tw, bands = tabs['h'].data_ptr(), tabs['w'].data_ptr(), tabs['tw'].data_ptr(), ctypes.addressof(tabs['bands'])

    def resample():
        assert lib.danet_stoi_resample(st, B, C, Ls, U, D, wav.data_ptr(), h, p['sig']) == 0

    def frames():
        assert lib.danet_stoi_frames(st, B, C, L10, p['sig'], win, p['E'], p['mask'], p['kidx'], p['M'], p['Emax']) == 0

    def bands_():
        assert lib.danet_stoi_bands(st, B, C, L10, p['sig'], win, tw, bands, p['kidx'], p['M'], p['T']) == 0

    def segments():
        assert lib.danet_stoi_segments(st, B, C, nf, p['T'], p['M'], p['d']) == 0

    def final():
        assert lib.danet_stoi_finalize(st, B, C, nf, p['d'], p['M'], p['Emax'], 0, B, p['per_utt'], p['perm_idx'],
                                       p['flags'], p['mean4'], p['count']) == 0

    def floor():
        assert lib.danet_stoi_finalize(st, 1, 1, nf, q['d'], q['M'], q['Emax'], 0, 1, q['per_utt'], q['perm_idx'],
                                       q['flags'], q['mean4'], q['count']) == 0
    fns = dict(resample=resample, frames=frames, bands=bands_, segments=segments, finalize=final, launch_floor=floor)
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    assert not w['flags'].any() and int(w['count']) == B
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    M = w['M'].cpu().numpy()
    r = dict(shape=dict(B=B, C=C, T=T, N=N, S=S, SMPRATE=SMPRATE), samples_per_signal=Ls, samples_at_10k=L10,
             frames_per_row=nf,
             kept_frames=dict(min=int(M.min()), max=int(M.max())), ffts_per_call=int(M.sum()) * (C + 2),
             unit='us per call, back to back, C entry point', mean4=[float(v) for v in w['mean4'].cpu()])
    r.update({k: _summary(v) for k, v in t.items()})
    print('stages: resample %.1f, frames %.1f, bands %.1f, segments %.1f, finalize %.1f us; launch floor %.1f us'
          % tuple(r[k]['median'] for k in fns), file=sys.stderr)

    # (b) the one bar: the whole device route against the host restatement of the same batch
    def route():
        return ops.stoi_eval(src, est, fft_stride=S, smprate=SMPRATE)
    out = route()
    torch.cuda.synchronize()
    dev = _summary([_timed_launches(route, reps) for _ in range(rounds)])
    wav_h = wav.cpu().numpy()
    h32 = tabs['h'].cpu().numpy()
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            rows = list(ex.map(lambda x: SR.evaluate(x, SMPRATE, h32), wav_h))
            ts.append((time.perf_counter() - t0) * 1e6)
    host = _summary(ts)
    per_h = np.stack([row[0] for row in rows])
    gap = float(np.abs(per_h - out[4].cpu().numpy()).max())
    r['route'] = dict(unit='us per batch', device=dev, host_restatement_16_threads=host,
                      speedup=round(host['median'] / dev['median'], 1), worst_abs_difference=gap,
                      device_is_faster=bool(dev['median'] + dev['spread'] < host['median'] - host['spread']))
    print('route: device %.0f us (spread %.0f), host restatement %.0f us (spread %.0f): x%.1f; worst |device - host| '
          '%.3g' % (dev['median'], dev['spread'], host['median'], host['spread'], r['route']['speedup'], gap),
          file=sys.stderr)
    return r


def valid_step_row(rounds, reps):
    import torch
    import bench
    from danet_amd.hparams import hparams
    from danet_amd.model import Model
    cfg = bench.CONFIGS['cfg2']
    base = dict(cfg['hp'], BATCH_SIZE=cfg['batch'], NUM_LSTM_LAYERS=cfg['layers'], LSTM_HDIM=cfg['hdim'],
                ENCODER_TYPE='bilstm-orig', OPTIMIZER_TYPE='adam')
    src = _spectra(cfg['batch'], cfg['hp']['MAX_N_SIGNAL'], cfg['frames'], 1)[0]
    assert src.shape[3] == cfg['hp']['FFT_SIZE'] // 2 + 1
    models = {}
    for tag, key in (('key_off', None), ('key_on', True)):
        hparams.reset()
        hparams.load(dict(base, EVAL_STOI=key))
        hparams.digest()
        models[tag] = Model('bench_stoi', device='cuda:0', seed=7).build()
    last = {}

    def step(tag):
        def fn():
            last[tag] = models[tag].valid_step(src)
        return fn
    for _ in range(3):
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
             key_on=_summary(t['key_on']),
             figures={k: float(last['key_on'][k]) for k in ('STOI', 'ESTOI', 'STOIi', 'ESTOIi')})
    r['added_us_per_step'] = round(r['key_on']['median'] - r['key_off']['median'], 2)
    print('valid_step: key off %.1f us (spread %.1f), key on %.1f us (spread %.1f): +%.1f us'
          % (r['key_off']['median'], r['key_off']['spread'], r['key_on']['median'], r['key_on']['spread'],
             r['added_us_per_step']), file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--step-reps', type=int, default=5)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_stoi.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='STOI / ESTOI / STOIi / ESTOIi of valid / test: resampling to 10 kHz, silent frames, band '
                        'magnitudes, segments, finalize; interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, step_reps=args.step_reps, device=torch.cuda.get_device_name(0))
    res['a_stages_cfg2'] = stages_row(args.rounds, args.reps)
    res['c_valid_step_cfg2'] = valid_step_row(args.rounds, args.step_reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'stoi_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if not res['a_stages_cfg2']['route']['device_is_faster']:
        sys.exit('the device route is not faster than the host restatement: see the route row')


if __name__ == '__main__':
    main()
