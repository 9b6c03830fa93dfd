'''
What the speed perturbation of the wavdir dataset (SPEED_PERTURB_RANGE) costs, measured in ONE process on one
box with INTERLEAVED blocks; prints one JSON line and writes it to profiles/speed_bench.json.  Every row
carries the per-block figures, their median and the block-to-block spread (max - min): a difference inside
the spread counts as equal.

  (a) danet_speed_resample alone on the cfg-2 batch shape -- 64 utterances of 8128 .. 40000 samples, speeds
      drawn at P = 0.1 -- through the C entry point, --reps back-to-back calls between two events per block,
      us per call; next to it the launch floor of the same run: the same entry point on one utterance of one
      sample;
  (b) WavDirData.epoch_device per batch at the cfg-2 shapes (64 utterances, crop to 128 frames) with the key at
      0.1 against the key null: host clock around whole epochs that end in a device synchronise, no consumer;
  (c) cli.train_epoch at cfg 2 with and without the key, ms per step incl. the feed.

No bar is set: nothing of this had been measured when the tool was written.  The WAV tree of (b) and (c) is
generated into a temporary folder.

    python tools/bench_speed.py [--rounds 7] [--reps 200] [--epochs 3] [--files 512] [--out FILE]
'''
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

P_RANGE = 0.1


def _summary(blocks):
    import numpy as np
    return dict(blocks=[round(float(v), 4) for v in blocks], median=round(float(np.median(blocks)), 4),
                spread=round(float(max(blocks) - min(blocks)), 4))


def _timed_launches(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per launch


def kernel_row(rounds, reps):
    import numpy as np
    import torch
    from danet_amd import _lib, datasets, ops
    rng = np.random.RandomState(0)
    lens = rng.randint(8128, 40001, size=64).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    p, out_lens = datasets.WavDirData.plan_speed(lens, rng, P_RANGE, 256)
    stride = (int(ops.speed_out_len(int(lens.max()), 512 - int(512 * P_RANGE))) + 3) & ~3
    spots = np.arange(64, dtype=np.int64) * stride
    pool = torch.randn(int(lens.sum()), device='cuda') * 1000.0
    out = torch.zeros(64 * stride, dtype=torch.float32, device='cuda')
    tab = torch.from_numpy(ops.speed_table(P_RANGE)).cuda()
    desc = ops.speed_desc(offs, lens, spots, out_lens, p, pool.numel(), out.numel())
    ops.speed_resample(pool, desc, tab, out)                    # (validates, maps the library)
    # one row against float64 on the host, so that the timed thing is known to be the right thing
    x = pool[:int(lens[0])].cpu().numpy()
    n = np.arange(int(out_lens[0]), dtype=np.int64)
    idx = (n * int(p[0]) // 512)[:, None] + np.arange(32)[None, :] - 15
    xw = np.where((idx >= 0) & (idx < len(x)), x[np.clip(idx, 0, len(x) - 1)], 0.0).astype(np.float64)
    prod = ops.speed_table(P_RANGE)[n * int(p[0]) % 512].astype(np.float64) * xw
    err = np.abs(out[:int(out_lens[0])].cpu().numpy() - prod.sum(axis=1)) / (np.abs(prod).sum(axis=1) + 1e-30)
    lib, st = _lib.load_speed(), _lib.stream()
    d64 = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    d1 = torch.from_numpy(ops.speed_desc([0], [1], [0], [1], [512], pool.numel(), out.numel()).view(np.uint8).copy()).cuda()
    one = torch.zeros(1, dtype=torch.float32, device='cuda')

    def cfg2():
        assert lib.danet_speed_resample(st, 64, pool.data_ptr(), pool.numel(), d64.data_ptr(), tab.data_ptr(),
                                        out.data_ptr(), out.numel()) == 0

    def tiny():
        assert lib.danet_speed_resample(st, 1, pool.data_ptr(), pool.numel(), d1.data_ptr(), tab.data_ptr(),
                                        one.data_ptr(), 1) == 0
    for _ in range(50):
        cfg2()
        tiny()
    torch.cuda.synchronize()
    t_cfg2, t_tiny = [], []
    for _ in range(rounds):
        t_cfg2.append(_timed_launches(cfg2, reps))
        t_tiny.append(_timed_launches(tiny, reps))
    macs = 32 * int(out_lens.sum())
    r = dict(utterances=64, samples_in=int(lens.sum()), samples_out=int(out_lens.sum()), multiply_adds=macs,
             unit='us per call, back to back, C entry point', max_err_over_bar_unit_row0=float(err.max() / (33 * 2.0 ** -24)),
             resample_64=_summary(t_cfg2), launch_floor_1x1=_summary(t_tiny))
    r['resample_64_GMACps'] = round(macs / (r['resample_64']['median'] * 1e-6) / 1e9, 1)
    print('resample 64 utterances (%.1f M multiply-adds): %.2f us (spread %.2f); one utterance of one sample: %.2f us '
          '(spread %.2f)' % (macs * 1e-6, r['resample_64']['median'], r['resample_64']['spread'],
                             r['launch_floor_1x1']['median'], r['launch_floor_1x1']['spread']), file=sys.stderr)
    return r


def feed_row(ds_off, ds_on, rounds, epochs):
    import torch
    from danet_amd.hparams import hparams
    bs = hparams.BATCH_SIZE * hparams.MAX_N_SIGNAL

    def run(ds):
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            for _batch in ds.epoch_device('train', bs, True, 'cuda', hparams.MAX_TRAIN_LEN):
                n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    run(ds_off)
    run(ds_on)
    t_off, t_on = [], []
    for _ in range(rounds):
        t_off.append(run(ds_off))
        t_on.append(run(ds_on))
    return dict(batch=bs, crop_frames=hparams.MAX_TRAIN_LEN, unit='ms per batch, host clock, no consumer',
                key_null=_summary(t_off), key_0_1=_summary(t_on))


def train_row(ds_off, ds_on, rounds, epochs):
    import torch
    from danet_amd import cli, feed
    from danet_amd.hparams import hparams
    from danet_amd.model import Model
    bs = hparams.BATCH_SIZE * hparams.MAX_N_SIGNAL
    model = Model('speed-bench', device='cuda', seed=1337).build()
    model.set_learn_rate(1e-4)

    def run(d):
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            _rep, k = cli.train_epoch(model, feed.EpochSource(d, 'train', bs, shuffle=True), io.StringIO())
            n += k
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    run(ds_off)
    run(ds_on)
    t_off, t_on = [], []
    for _ in range(rounds):
        t_off.append(run(ds_off))
        t_on.append(run(ds_on))
    model.check_status()
    return dict(unit='ms per train step incl. the feed, host clock', key_null=_summary(t_off), key_0_1=_summary(t_on))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--files', type=int, default=512)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    import bench
    import bench_prep
    from danet_amd import datasets
    from danet_amd.hparams import hparams
    assert torch.cuda.is_available(), 'bench_speed.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='wavdir speed perturbation: the resampling kernel, the feed and the train epoch with the key '
                        'at %g against null; interleaved blocks in one process' % P_RANGE,
               rounds=args.rounds, reps=args.reps, device=torch.cuda.get_device_name(0))
    res['a_resample_cfg2_batch'] = kernel_row(args.rounds, args.reps)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'tree')
        bench_prep.write_tree(root, args.files)
        cfg = bench.CONFIGS['cfg2']
        base = dict(cfg['hp'], BATCH_SIZE=cfg['batch'], NUM_LSTM_LAYERS=cfg['layers'], LSTM_HDIM=cfg['hdim'],
                    MAX_TRAIN_LEN=cfg['frames'], ENCODER_TYPE='bilstm-orig', OPTIMIZER_TYPE='adam',
                    DATASET_TYPE='wavdir', DATASET_DIR=root)
        made = []
        for keys in (dict(), dict(SPEED_PERTURB_RANGE=P_RANGE)):
            hparams.reset()
            hparams.load(dict(base, **keys))
            hparams.digest()
            ds = datasets.WavDirData()
            ds.load_host(out=sys.stderr)
            ds.is_loaded = True
            made.append(ds)
        r = res['b_epoch_device_cfg2'] = feed_row(made[0], made[1], args.rounds, args.epochs)
        r['added_us_per_batch'] = round((r['key_0_1']['median'] - r['key_null']['median']) * 1e3, 2)
        t = res['c_train_epoch_cfg2'] = train_row(made[0], made[1], args.rounds, args.epochs)
        t['added_us_per_step'] = round((t['key_0_1']['median'] - t['key_null']['median']) * 1e3, 2)
    print('epoch_device per batch: key null %.4f ms (spread %.4f), key 0.1 %.4f ms (spread %.4f): %+.1f us'
          % (r['key_null']['median'], r['key_null']['spread'], r['key_0_1']['median'], r['key_0_1']['spread'],
             r['added_us_per_batch']), file=sys.stderr)
    print('train_epoch per step: key null %.4f ms (spread %.4f), key 0.1 %.4f ms (spread %.4f): %+.1f us'
          % (t['key_null']['median'], t['key_null']['spread'], t['key_0_1']['median'], t['key_0_1']['spread'],
             t['added_us_per_step']), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'speed_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
