'''
What the mixture level control of the wavdir dataset (MIX_SNR_RANGE / MIX_LEVEL_RANGE) costs, measured in
ONE process on one box with INTERLEAVED blocks; prints one JSON line and writes it to
profiles/mix_bench.json.  Every row carries the per-block figures, their median and the block-to-block
spread (max - min): a difference inside the spread counts as equal.

  (a) danet_mix_power over a synthetic pool of mixed lengths (--rows utterances of 1 .. 10 s at 8 kHz plus
      two of 5e6 samples, laid back to back): --reps back-to-back calls through the C entry point between two
      events per block, us per call and GB/s against the pool's size; next to it, as a yardstick of the same
      run, torch's float32 `pool.square().sum()` over the same bytes (one pass, no per-row results);
  (b) WavDirData.epoch_device per batch at the cfg-2 shapes (64 utterances, crop to 128 frames) with both keys
      set against both keys null: host clock around whole epochs that end in a device synchronise, no
      consumer, ms per batch; and the launch floor of the same run: danet_mix_scale_c64 on a [1][1][1] batch,
      back to back between two events.

The bar of (b): the added time per batch (keys set - keys null, medians) is no more than TWO launch floors.
(a) is reported.  The WAV tree of (b) is generated into a temporary folder.

    python tools/bench_mix.py [--rounds 7] [--reps 20] [--epochs 3] [--files 512] [--rows 2000] [--out FILE]
'''
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


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


def power_row(n_rows, rounds, reps):
    import numpy as np
    import torch
    from danet_amd import _lib, ops
    rng = np.random.RandomState(0)
    lens = np.concatenate([rng.randint(8000, 80001, size=n_rows), [5 * 10 ** 6, 5 * 10 ** 6]]).astype(np.int64)
    rng.shuffle(lens)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    total = int(lens.sum())
    pool = torch.empty(total, dtype=torch.float32, device='cuda')
    for lo in range(0, total, 1 << 24):
        pool[lo:lo + (1 << 24)] = torch.randn(min(1 << 24, total - lo), device='cuda') * 1000.0
    got = ops.mix_power(pool, offs, lens)                       # (validates, maps the library)
    # accuracy on a few rows against float64, so that the timed thing is known to be the right thing
    err = 0.0
    for u in (0, 1, int(np.argmax(lens))):
        x = pool[int(offs[u]):int(offs[u] + lens[u])].double()
        want = float((x * x).sum())
        err = max(err, abs(float(got[u]) - want) / want)
    lib, st = _lib.load_mix(), _lib.stream()
    o, l = torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda()
    max_len = int(lens.max())
    nbytes = lib.danet_mix_workspace_bytes(len(lens), max_len)
    ws = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device='cuda')
    out = torch.empty(len(lens), dtype=torch.float64, device='cuda')
    args = (st, len(lens), pool.data_ptr(), total, o.data_ptr(), l.data_ptr(), max_len, out.data_ptr(), ws.data_ptr(),
            nbytes)

    def new():
        assert lib.danet_mix_power(*args) == 0

    def yard():
        pool.square().sum()
    for _ in range(3):
        new()
        yard()
    torch.cuda.synchronize()
    assert torch.equal(out, got)                                # two routes, bit for bit
    t_new, t_yard = [], []
    for _ in range(rounds):
        t_new.append(_timed_launches(new, reps))
        t_yard.append(_timed_launches(yard, reps))
    r = dict(rows=len(lens), samples=total, pool_bytes=4 * total, longest_row=max_len, shortest_row=int(lens.min()),
             launches_per_call=2 if nbytes else 1, workspace_bytes=int(nbytes), unit='us per call, C entry point',
             max_rel_err_vs_float64_on_3_rows=err, mix_power=_summary(t_new),
             torch_square_sum_f32=_summary(t_yard))
    r['mix_power_GBps'] = round(4 * total / (r['mix_power']['median'] * 1e-6) / 1e9, 1)
    r['torch_square_sum_f32_GBps'] = round(4 * total / (r['torch_square_sum_f32']['median'] * 1e-6) / 1e9, 1)
    print('power: %d rows, %.1f MB: %.1f us (spread %.1f) = %.0f GB/s; torch square().sum(): %.1f us = %.0f GB/s'
          % (len(lens), 4e-6 * total, r['mix_power']['median'], r['mix_power']['spread'], r['mix_power_GBps'],
             r['torch_square_sum_f32']['median'], r['torch_square_sum_f32_GBps']), file=sys.stderr)
    return r


def floor_row(rounds, reps):
    import torch
    from danet_amd import _lib
    lib, st = _lib.load_mix(), _lib.stream()
    buf = torch.zeros(2, dtype=torch.float32, device='cuda')
    g = torch.ones(1, dtype=torch.float32, device='cuda')
    big = torch.zeros(64 * 128 * 129 * 2, dtype=torch.float32, device='cuda')
    g64 = torch.ones(64, dtype=torch.float32, device='cuda')

    def tiny():
        assert lib.danet_mix_scale_c64(st, 1, 1, 1, buf.data_ptr(), 1, g.data_ptr()) == 0

    def cfg2():
        assert lib.danet_mix_scale_c64(st, 64, 128, 129, big.data_ptr(), 129, g64.data_ptr()) == 0
    for _ in range(50):
        tiny()
        cfg2()
    torch.cuda.synchronize()
    t_tiny, t_cfg2 = [], []
    for _ in range(rounds):
        t_tiny.append(_timed_launches(tiny, reps))
        t_cfg2.append(_timed_launches(cfg2, reps))
    return dict(unit='us per launch, back to back, C entry point', scale_1x1x1=_summary(t_tiny),
                scale_64x128x129=_summary(t_cfg2))


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
                keys_null=_summary(t_off), keys_set=_summary(t_on))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--files', type=int, default=512)
    ap.add_argument('--rows', type=int, default=2000)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    import bench
    import bench_prep
    from danet_amd import datasets
    from danet_amd.hparams import hparams
    assert torch.cuda.is_available(), 'bench_mix.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='wavdir mixture levels: per-utterance power of a pool, per-batch gains; interleaved blocks '
                        'in one process', rounds=args.rounds, reps=args.reps, device=torch.cuda.get_device_name(0))
    res['a_power_mixed_pool'] = power_row(args.rows, args.rounds, args.reps)
    res['launch_floor'] = floor_row(args.rounds, 200)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'tree')
        bench_prep.write_tree(root, args.files)
        cfg = bench.CONFIGS['cfg2']
        base = dict(cfg['hp'], BATCH_SIZE=cfg['batch'], NUM_LSTM_LAYERS=cfg['layers'], LSTM_HDIM=cfg['hdim'],
                    MAX_TRAIN_LEN=cfg['frames'], ENCODER_TYPE='bilstm-orig', OPTIMIZER_TYPE='adam',
                    DATASET_TYPE='wavdir', DATASET_DIR=root)
        made = []
        for keys in (dict(), dict(MIX_SNR_RANGE=5.0, MIX_LEVEL_RANGE=3.0)):
            hparams.reset()
            hparams.load(dict(base, **keys))
            hparams.digest()
            ds = datasets.WavDirData()
            ds.load_host(out=sys.stderr)
            ds.is_loaded = True
            made.append(ds)
        r = res['b_epoch_device_cfg2'] = feed_row(made[0], made[1], args.rounds, args.epochs)
    floor_us = res['launch_floor']['scale_1x1x1']['median']
    r['added_us_per_batch'] = round((r['keys_set']['median'] - r['keys_null']['median']) * 1e3, 2)
    r['launch_floor_us'] = floor_us
    r['bar'] = 'added_us_per_batch <= 2 * launch_floor_us'
    r['bar_met'] = bool(r['added_us_per_batch'] <= 2 * floor_us)
    print('epoch_device per batch: keys null %.4f ms (spread %.4f), keys set %.4f ms (spread %.4f): +%.1f us; launch '
          'floor %.2f us; bar (<= 2 floors) met: %s' % (r['keys_null']['median'], r['keys_null']['spread'],
                                                         r['keys_set']['median'], r['keys_set']['spread'],
                                                         r['added_us_per_batch'], floor_us, r['bar_met']), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'mix_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
