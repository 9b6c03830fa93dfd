'''
What the additive noise of the wavdir dataset (NOISE_DIR, NOISE_SNR_MIN, NOISE_SNR_MAX) costs, measured in ONE
process on one box with INTERLEAVED blocks; prints one JSON line and writes it to profiles/noise_bench.json.  Every
row carries the per-block figures, their median and the block-to-block spread (max - min): a difference inside the
spread counts as equal.

  (a) danet_noise_frontend_fwd alone through the C entry point at the cfg-2 shape (B = 32, C = 2, N = 128 * 129),
      --reps back-to-back calls between two events per block, us per call; beside it in the same run the core
      kernel danet_frontend_fwd at C = 2 and at C = 3 (the same inputs plus one more src_pwr row: the BAR is "not
      slower than that one") and the launch floor (the new entry point at B = C = N = 1);
  (b) WavDirData.epoch_device per batch at the cfg-2 shapes with the keys set against null;
  (c) cli.train_epoch at cfg 2 with and without the keys, ms per step incl. the feed.

(b) and (c) are measured by the routines of tools/bench_speed.py on a generated WAV tree and generated noise files.

    python tools/bench_noise.py [--rounds 7] [--reps 200] [--epochs 3] [--files 512] [--kernel-only] [--out FILE]
'''
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SNR = (0.0, 20.0)


def kernel_rows(rounds, reps):
    import torch
    import bench_speed
    from danet_amd import _lib, ops
    B, C, T, F = 32, 2, 128, 129
    N = T * F
    g = torch.Generator(device='cuda').manual_seed(0)
    rows = torch.view_as_complex(torch.randn(B, C + 1, T, F, 2, device='cuda', generator=g) * 50)
    src = rows[:, :C].contiguous()
    noise = rows[:, C].contiguous()
    gain = torch.rand(B, device='cuda', generator=g) * 2
    scaled = torch.cat([src, torch.view_as_complex((torch.view_as_real(noise) * gain.view(B, 1, 1, 1)).contiguous())
                        [:, None]], dim=1).contiguous()
    f = lambda *s: torch.empty(*s, device='cuda')
    mix_pwr, mix_log, phasor, src_pwr, src_pwr3 = f(B, N), f(B, N), f(B, N, 2), f(B, C, N), f(B, C + 1, N)
    one = [f(2) for _ in range(6)]
    lib, core, st = _lib.load_noise(), _lib.load(), _lib.stream()
    p = lambda t: (torch.view_as_real(t) if t.is_complex() else t).data_ptr()

    def new():
        assert lib.danet_noise_frontend_fwd(st, B, C, N, p(src), p(noise), p(gain), p(mix_pwr), p(mix_log), p(phasor),
                                            p(src_pwr), None) == 0

    def core_c(c, x, sp):
        def fn():
            assert core.danet_frontend_fwd(st, B, c, N, p(x), p(mix_pwr), p(mix_log), p(phasor), None, p(sp), None) == 0
        return fn

    def floor():
        assert lib.danet_noise_frontend_fwd(st, 1, 1, 1, p(one[0]), p(one[1]), None, p(one[2]), p(one[3]), p(one[4]),
                                            p(one[5]), None) == 0
    fns = dict(noise_c2=new, core_c2=core_c(C, src, src_pwr), core_c3=core_c(C + 1, scaled, src_pwr3), floor=floor)
    # the timed thing is the right thing: bit for bit the core kernel on C + 1 rows
    want = ops.frontend(scaled)
    got = ops.noise_frontend(src, noise, gain)
    exact = all(bool((got[k].view(torch.int32) == (want[k][:, :C] if k == 'src_pwr' else want[k]).view(torch.int32)).all())
                for k in ('src_pwr', 'mix_pwr', 'mix_log', 'phasor'))
    for _ in range(20):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(bench_speed._timed_launches(fn, reps))
    moved = 8 * B * (C + 1) * N + 4 * B * N * (C + 4)
    r = dict(B=B, C=C, N=N, unit='us per call, back to back, C entry point', equals_core_on_C_plus_1_rows=exact,
             bytes_moved=moved)
    for k in fns:
        r[k] = bench_speed._summary(t[k])
    r['noise_c2_GBps'] = round(moved / (r['noise_c2']['median'] * 1e-6) / 1e9, 1)
    d = r['noise_c2']['median'] - r['core_c3']['median']
    r['noise_minus_core_c3_us'] = round(d, 2)
    r['bar_not_slower_than_core_c3'] = bool(d <= max(r['noise_c2']['spread'], r['core_c3']['spread']))
    print('noise front-end %.2f us (spread %.2f), core C=2 %.2f us, core C=3 %.2f us (spread %.2f), floor %.2f us; '
          'equal to the core kernel bit for bit: %s' % (r['noise_c2']['median'], r['noise_c2']['spread'],
                                                        r['core_c2']['median'], r['core_c3']['median'],
                                                        r['core_c3']['spread'], r['floor']['median'], exact),
          file=sys.stderr)
    return r


def write_noise(folder, n_files=8, seed=3):
    import numpy as np
    import scipy.io.wavfile
    rng = np.random.RandomState(seed)
    os.makedirs(folder, exist_ok=True)
    for i in range(n_files):
        n = int(rng.uniform(1.0, 30.0) * 8000)
        w = rng.randn(n) * 30.0 * 200.0 ** rng.uniform(0, 1)
        scipy.io.wavfile.write(os.path.join(folder, 'noise%02d.wav' % i), 8000,
                               np.clip(w, -32768, 32767).astype(np.int16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--files', type=int, default=512)
    ap.add_argument('--kernel-only', action='store_true', help='measure (a) only')
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    import bench
    import bench_prep
    import bench_speed
    from danet_amd import datasets
    from danet_amd.hparams import hparams
    assert torch.cuda.is_available(), 'bench_noise.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='wavdir additive noise: the front-end kernel, the feed and the train epoch with the keys set '
                        '(SNR %g .. %g dB) against null; interleaved blocks in one process' % SNR,
               rounds=args.rounds, reps=args.reps, device=torch.cuda.get_device_name(0))
    res['a_frontend_cfg2'] = kernel_rows(args.rounds, args.reps)
    if not args.kernel_only:
        with tempfile.TemporaryDirectory() as tmp:
            root, noise = os.path.join(tmp, 'tree'), os.path.join(tmp, 'noise')
            bench_prep.write_tree(root, args.files)
            write_noise(noise)
            cfg = bench.CONFIGS['cfg2']
            base = dict(cfg['hp'], BATCH_SIZE=cfg['batch'], NUM_LSTM_LAYERS=cfg['layers'], LSTM_HDIM=cfg['hdim'],
                        MAX_TRAIN_LEN=cfg['frames'], ENCODER_TYPE='bilstm-orig', OPTIMIZER_TYPE='adam',
                        DATASET_TYPE='wavdir', DATASET_DIR=root)
            made = []
            for keys in (dict(), dict(NOISE_DIR=noise, NOISE_SNR_MIN=SNR[0], NOISE_SNR_MAX=SNR[1])):
                hparams.reset()
                hparams.load(dict(base, **keys))
                hparams.digest()
                ds = datasets.WavDirData()
                ds.load_host(out=sys.stderr)
                ds.is_loaded = True
                made.append(ds)
            for name, row in (('b_epoch_device_cfg2', bench_speed.feed_row(made[0], made[1], args.rounds, args.epochs)),
                              ('c_train_epoch_cfg2', bench_speed.train_row(made[0], made[1], args.rounds, args.epochs))):
                row['keys_set'] = row.pop('key_0_1')                # (the routines of bench_speed.py name their own key)
                row['added_us'] = round((row['keys_set']['median'] - row['key_null']['median']) * 1e3, 2)
                res[name] = row
                print('%s: keys null %.4f ms (spread %.4f), keys set %.4f ms (spread %.4f): %+.1f us'
                      % (name, row['key_null']['median'], row['key_null']['spread'], row['keys_set']['median'],
                         row['keys_set']['spread'], row['added_us']), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'noise_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
