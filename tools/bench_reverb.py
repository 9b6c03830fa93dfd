'''
What the reverberation of the wavdir dataset (REVERB_RT60_MAX) costs, measured in ONE process on one box with
INTERLEAVED blocks; prints one JSON line and writes it to profiles/reverb_bench.json.  Every row carries the
per-block figures, their median and the block-to-block spread (max - min): a difference inside the spread counts
as equal.

  (a) danet_reverb_apply alone through the C entry point on the cfg-2 CROPPED shape -- 64 rows with spans of
      128 * 64 + 256 samples inside utterances of 8128 .. 40000 samples, mixed bank rows -- at K = 4000 and at
      K = 800, --reps back-to-back calls between two events per block, us per call and TFLOP/s (2 K flop per
      output sample); next to it the launch floor of the same run: the same entry point on one row, one sample,
      K = 4;
  (b) WavDirData.epoch_device per batch at the cfg-2 shapes with the key at 0.5 against the key null;
  (c) cli.train_epoch at cfg 2 with and without the key, ms per step incl. the feed.

No bar is set for (a); the README reports it beside the 52 TFLOP/s of a tuned fp32 VALU kernel.  (b) and (c) are
measured by the routines of tools/bench_speed.py on a generated WAV tree.

    python tools/bench_reverb.py [--rounds 7] [--reps 50] [--epochs 3] [--files 512] [--out FILE]
'''
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

RT60 = 0.5
SPAN = 128 * 64 + 256


def kernel_rows(rounds, reps):
    import numpy as np
    import torch
    import bench_speed
    from danet_amd import _lib, ops
    rng = np.random.RandomState(0)
    lens = rng.randint(8128, 40001, size=64).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    first = np.asarray([rng.randint(0, int(l) - SPAN + 1) if l > SPAN else 0 for l in lens], dtype=np.int64)
    count = np.minimum(lens - first, SPAN)
    rows = rng.randint(0, ops.REVERB_ROWS, size=64).astype(np.int64)
    stride = (int(lens.max()) + 3) & ~3
    spots = np.arange(64, dtype=np.int64) * stride
    pool = torch.randn(int(lens.sum()), device='cuda') * 1000.0
    out = torch.zeros(64 * stride, dtype=torch.float32, device='cuda')
    desc = ops.reverb_desc(offs, lens, spots, first, count, rows, pool.numel(), out.numel())
    d64 = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    d1 = torch.from_numpy(ops.reverb_desc([0], [1], [0], [0], [1], [0], pool.numel(), out.numel()).view(np.uint8).copy()).cuda()
    lib, st = _lib.load_reverb(), _lib.stream()
    banks = {K: torch.from_numpy(ops.reverb_bank((K - 2) / 8000.0, 8000)).cuda() for K in (4000, 800, 4)}
    assert all(b.shape == (ops.REVERB_ROWS, K) for K, b in banks.items())

    def call(K, n, d):
        def fn():
            assert lib.danet_reverb_apply(st, n, pool.data_ptr(), pool.numel(), d.data_ptr(), banks[K].data_ptr(), K,
                                          out.data_ptr(), out.numel()) == 0
        return fn
    fns = dict(k4000=call(4000, 64, d64), k800=call(800, 64, d64), floor=call(4, 1, d1))
    # one row against float64 on the host, so that the timed thing is known to be the right thing
    fns['k4000']()
    torch.cuda.synchronize()
    x = pool[int(offs[0]):int(offs[0] + lens[0])].cpu().numpy().astype(np.float64)
    h = banks[4000][int(rows[0])].cpu().numpy().astype(np.float64)
    lo, n = int(first[0]), int(count[0])
    y64 = np.convolve(x, h)[lo:lo + n]
    S = np.convolve(np.abs(x), np.abs(h))[lo:lo + n]
    err = np.abs(out[lo:lo + n].cpu().numpy() - y64) / (1.01 * 4000 * 2.0 ** -24 * S + 1e-30)
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(bench_speed._timed_launches(fn, reps if k != 'floor' else 4 * reps))
    r = dict(rows=64, span_samples=int(count.sum()), unit='us per call, back to back, C entry point',
             max_err_over_bar_row0=float(err.max()), launch_floor_1_row_1_sample_K4=bench_speed._summary(t['floor']))
    for k, K in (('k4000', 4000), ('k800', 800)):
        s = bench_speed._summary(t[k])
        s['TFLOPs'] = round(2.0 * K * int(count.sum()) / (s['median'] * 1e-6) / 1e12, 2)
        r['apply_64_K%d' % K] = s
        print('apply 64 rows K = %d: %.1f us (spread %.1f), %.2f TFLOP/s' % (K, s['median'], s['spread'], s['TFLOPs']),
              file=sys.stderr)
    print('launch floor: %.2f us' % r['launch_floor_1_row_1_sample_K4']['median'], file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50)
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
    assert torch.cuda.is_available(), 'bench_reverb.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='wavdir reverberation: the FIR kernel, the feed and the train epoch with the key at %g against '
                        'null; interleaved blocks in one process' % RT60,
               rounds=args.rounds, reps=args.reps, device=torch.cuda.get_device_name(0))
    res['a_apply_cfg2_cropped'] = kernel_rows(args.rounds, args.reps)
    if not args.kernel_only:
        with tempfile.TemporaryDirectory() as tmp:
            root = os.path.join(tmp, 'tree')
            bench_prep.write_tree(root, args.files)
            cfg = bench.CONFIGS['cfg2']
            base = dict(cfg['hp'], BATCH_SIZE=cfg['batch'], NUM_LSTM_LAYERS=cfg['layers'], LSTM_HDIM=cfg['hdim'],
                        MAX_TRAIN_LEN=cfg['frames'], ENCODER_TYPE='bilstm-orig', OPTIMIZER_TYPE='adam',
                        DATASET_TYPE='wavdir', DATASET_DIR=root)
            made = []
            for keys in (dict(), dict(REVERB_RT60_MAX=RT60)):
                hparams.reset()
                hparams.load(dict(base, **keys))
                hparams.digest()
                ds = datasets.WavDirData()
                ds.load_host(out=sys.stderr)
                ds.is_loaded = True
                made.append(ds)
            for name, row in (('b_epoch_device_cfg2', bench_speed.feed_row(made[0], made[1], args.rounds, args.epochs)),
                              ('c_train_epoch_cfg2', bench_speed.train_row(made[0], made[1], args.rounds, args.epochs))):
                row['key_0_5'] = row.pop('key_0_1')                 # (the routines of bench_speed.py name their own key)
                row['added_us'] = round((row['key_0_5']['median'] - row['key_null']['median']) * 1e3, 2)
                res[name] = row
                print('%s: key null %.4f ms (spread %.4f), key 0.5 %.4f ms (spread %.4f): %+.1f us'
                      % (name, row['key_null']['median'], row['key_null']['spread'], row['key_0_5']['median'],
                         row['key_0_5']['spread'], row['added_us']), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'reverb_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
