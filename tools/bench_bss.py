'''
What the BSS-eval figures of valid / test (EVAL_BSS_SDR) cost, measured in ONE process on one box with INTERLEAVED
blocks; prints one JSON line and writes it to profiles/bss_bench.json.  Every row carries the per-block figures,
their median and the block-to-block spread (max - min): a difference inside the spread counts as equal.

  (a) the stages at the cfg-2 validation shape (B = 32, C = 2, T = 128, N = 256, S = 64, L = 512): --reps
      back-to-back calls through the C entry point between two events per block, us per call, next to the launch
      floor of the same run (danet_bss_finalize on one utterance of one source, L = 1).  xcorr as float64 GFLOP/s.
      The Cholesky solve works in place, so each timed call is preceded by a device copy that restores the
      matrices; the copy is timed alone in the same blocks and its median is subtracted.
  (b) danet_bss_chol_solve at n = 1024, nmat = 32 and n = 512, nmat = 64 as GFLOP/s (n^3 / 3 per matrix), next to
      float64 torch.linalg.cholesky + torch.cholesky_solve on the same matrices on the device (if the installed torch
      provides them there) and scipy.linalg.cho_factor / cho_solve over the batch on the host with 16 threads.
      Yardsticks only.
  (c) the whole device route for the batch (ops.bss_eval from spectra: synthesis and the five stages) against the host
      restatement (b) of tests/bss_ref.py on the same waveforms with 16 threads.  THE ONE BAR: the device route must be
      faster, otherwise the library has no reason to exist.
  (d) Model.valid_step at cfg 2 with the key on against the key off.

    python tools/bench_bss.py [--rounds 5] [--reps 5] [--step-reps 5] [--out FILE]
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


def _spectra(B, C, T, F, seed):
    import numpy as np
    import torch
    rng = np.random.RandomState(seed)
    z = lambda: rng.randn(B, C, T, F) + 1j * rng.randn(B, C, T, F)
    src = z()
    est = src + 0.3 * src[:, ::-1] + 0.5 * z()
    return torch.from_numpy(src.astype(np.complex64)).cuda(), torch.from_numpy(est.astype(np.complex64)).cuda()


def stages_row(rounds, reps, B=32, C=2, T=128, N=256, S=64, L=512):
    import numpy as np
    import torch
    import bss_ref as BR
    from danet_amd import _lib, ops
    from danet_amd.hparams import hparams
    hparams.reset()
    hparams.load(dict(FFT_SIZE=N, FFT_STRIDE=S))
    hparams.digest()
    src, est = _spectra(B, C, T, N // 2 + 1, 0)
    Ls, n = (T - 1) * S, C * L
    wav = ops.metric_synth(src, est, S)
    lib, st = _lib.load_bss(), _lib.stream()
    w = {name: torch.zeros(shape, dtype=dtype, device='cuda') for name, shape, dtype in ops.bss_parts(B, C, L)}
    p = {k: v.data_ptr() for k, v in w.items()}
    one = {name: torch.zeros(shape, dtype=dtype, device='cuda') for name, shape, dtype in ops.bss_parts(1, 1, 1)}
    q = {k: v.data_ptr() for k, v in one.items()}

    def xcorr():
        assert lib.danet_bss_xcorr(st, B, C, Ls, L, wav.data_ptr(), p['R'], p['D'], p['ee']) == 0

    def systems():
        assert lib.danet_bss_systems(st, B, C, L, p['R'], p['D'], p['G'], p['Gs'], p['Xg'], p['Xs']) == 0
    xcorr()
    systems()
    G0, Gs0, Xg0, Xs0 = w['G'].clone(), w['Gs'].clone(), w['Xg'].clone(), w['Xs'].clone()

    def restore_big():
        w['G'].copy_(G0)
        w['Xg'].copy_(Xg0)

    def restore_small():
        w['Gs'].copy_(Gs0)
        w['Xs'].copy_(Xs0)

    def chol_big():
        restore_big()
        assert lib.danet_bss_chol_solve(st, B, n, C, p['G'], p['Xg'], p['fg']) == 0

    def chol_small():
        restore_small()
        assert lib.danet_bss_chol_solve(st, B * C, L, C + 1, p['Gs'], p['Xs'], p['fs']) == 0

    def final():
        assert lib.danet_bss_finalize(st, B, C, L, p['R'], p['D'], p['ee'], p['Xg'], p['Xs'], p['fg'], p['fs'], 0, B,
                                      p['per_utt'], p['perm_idx'], p['flags'], p['mean4']) == 0

    def floor():
        assert lib.danet_bss_finalize(st, 1, 1, 1, q['R'], q['D'], q['ee'], q['Xg'], q['Xs'], q['fg'], q['fs'], 0, 1,
                                      q['per_utt'], q['perm_idx'], q['flags'], q['mean4']) == 0
    fns = dict(xcorr=xcorr, systems=systems, restore_1024x32=restore_big, chol_1024x32_with_restore=chol_big,
               restore_512x64=restore_small, chol_512x64_with_restore=chol_small, finalize=final, launch_floor=floor)
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    assert not w['fg'].any() and not w['fs'].any() and not w['flags'].any()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    r = dict(shape=dict(B=B, C=C, T=T, N=N, S=S, L=L), samples_per_signal=Ls,
             unit='us per call, back to back, C entry point', mean4_db=[float(v) for v in w['mean4'].cpu()])
    r.update({k: _summary(v) for k, v in t.items()})
    lags = C * (C + 1) // 2 * (2 * L - 1) - C * (L - 1) + C * C * L + C     # the lags one utterance computes
    r['xcorr_gflops'] = round(2.0 * B * lags * Ls / r['xcorr']['median'] * 1e-3, 1)
    for tag, nm, nn in (('1024x32', B, n), ('512x64', B * C, L)):
        us = r['chol_%s_with_restore' % tag]['median'] - r['restore_%s' % tag]['median']
        r['chol_%s_us' % tag] = round(us, 1)
        r['chol_%s_gflops' % tag] = round(nm * nn ** 3 / 3.0 / us * 1e-3, 1)
    print('stages: xcorr %.0f us (%.0f GFLOP/s), systems %.0f, chol 1024x32 %.0f (%.0f GFLOP/s), chol 512x64 %.0f '
          '(%.0f GFLOP/s), finalize %.0f us; launch floor %.1f us'
          % (r['xcorr']['median'], r['xcorr_gflops'], r['systems']['median'], r['chol_1024x32_us'],
             r['chol_1024x32_gflops'], r['chol_512x64_us'], r['chol_512x64_gflops'], r['finalize']['median'],
             r['launch_floor']['median']), file=sys.stderr)

    # (b) yardsticks on the same matrices
    yard = {}
    for tag, A0, X0 in (('1024x32', G0, Xg0), ('512x64', Gs0.view(B * C, L, L), Xs0.view(B * C, C + 1, L))):
        nm, nn = A0.shape[0], A0.shape[1]
        try:
            def torch_route():
                torch.cholesky_solve(X0.transpose(1, 2), torch.linalg.cholesky(A0))
            torch_route()
            torch.cuda.synchronize()
            us = _summary([_timed_launches(torch_route, max(1, reps // 2)) for _ in range(rounds)])
            yard['torch_' + tag] = dict(us, gflops=round(nm * nn ** 3 / 3.0 / us['median'] * 1e-3, 1))
        except Exception as e:                                   # not provided on this device: say so
            yard['torch_' + tag] = dict(unavailable=str(e)[:200])
        import scipy.linalg
        A_h, X_h = A0.cpu().numpy(), X0.cpu().numpy()

        def host_one(m):
            return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A_h[m], lower=True, check_finite=False), X_h[m].T,
                                          check_finite=False)
        with ThreadPoolExecutor(HOST_THREADS) as ex:
            list(ex.map(host_one, range(nm)))
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                list(ex.map(host_one, range(nm)))
                ts.append((time.perf_counter() - t0) * 1e6)
        us = _summary(ts)
        yard['scipy_%d_threads_%s' % (HOST_THREADS, tag)] = dict(us, gflops=round(nm * nn ** 3 / 3.0 / us['median'] * 1e-3, 1))
    r['yardsticks'] = yard
    print('yardsticks: %s' % {k: v.get('median', v.get('unavailable')) for k, v in yard.items()}, file=sys.stderr)

    # (c) the one bar: the whole device route against the host restatement of the same batch
    def route():
        return ops.bss_eval(src, est, filter_len=L, fft_stride=S)
    out = route()
    torch.cuda.synchronize()
    dev = _summary([_timed_launches(route, reps) for _ in range(rounds)])
    wav_h = wav.cpu().numpy()
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            rows = list(ex.map(lambda x: BR.evaluate(x, L), wav_h))
            ts.append((time.perf_counter() - t0) * 1e6)
    host = _summary(ts)
    per_h = np.stack([row[0] for row in rows])
    gap = float(np.abs(per_h - out[4].cpu().numpy()).max())
    r['route'] = dict(unit='us per batch', device=dev, host_restatement_16_threads=host,
                      speedup=round(host['median'] / dev['median'], 1), worst_abs_difference_db=gap,
                      device_is_faster=bool(dev['median'] + dev['spread'] < host['median'] - host['spread']))
    print('route: device %.0f us (spread %.0f), host restatement %.0f us (spread %.0f): x%.1f; worst |device - host| '
          '%.3g dB' % (dev['median'], dev['spread'], host['median'], host['spread'], r['route']['speedup'], gap),
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
    models = {}
    for tag, key in (('key_off', None), ('key_on', True)):
        hparams.reset()
        hparams.load(dict(base, EVAL_BSS_SDR=key))
        hparams.digest()
        models[tag] = Model('bench_bss', device='cuda:0', seed=7).build()
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
             key_on=_summary(t['key_on']), figures_db={k: float(last['key_on'][k]) for k in ('SDR', 'SIR', 'SAR', 'SDRi')})
    r['added_us_per_step'] = round(r['key_on']['median'] - r['key_off']['median'], 2)
    print('valid_step: key off %.1f us (spread %.1f), key on %.1f us (spread %.1f): +%.1f us'
          % (r['key_off']['median'], r['key_off']['spread'], r['key_on']['median'], r['key_on']['spread'],
             r['added_us_per_step']), file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--step-reps', type=int, default=5)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_bss.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='BSS-eval SDR / SIR / SAR / SDRi of valid / test: correlations, systems, blocked Cholesky '
                        'solves, finalize; interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, step_reps=args.step_reps, device=torch.cuda.get_device_name(0))
    res['a_stages_cfg2'] = stages_row(args.rounds, args.reps)
    res['d_valid_step_cfg2'] = valid_step_row(args.rounds, args.step_reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'bss_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if not res['a_stages_cfg2']['route']['device_is_faster']:
        sys.exit('the device route is not faster than the host restatement: see the route row')


if __name__ == '__main__':
    main()
