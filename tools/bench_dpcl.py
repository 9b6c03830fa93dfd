'''
What the deep-clustering auxiliary loss (DPCL_WEIGHT) costs, measured in ONE process on one box with INTERLEAVED
blocks; prints one JSON line and writes it to profiles/dpcl_bench.json.  Every row carries the per-block figures,
their median and the block-to-block spread (max - min): a difference inside the spread counts as equal.

  (1) danet_dpcl_stats, danet_dpcl_finalize and danet_dpcl_bwd alone through the C ABI at (B, N, E, C) =
      (32, 16512, 20, 2) and (32, 16512, 40, 3): --reps back-to-back calls between two events per block, us per call;
  (2) the launch floor of the same run (danet_dpcl_bwd at B = N = E = C = 1);
  (3) a device copy of exactly the bytes each big pass must move, as the yardstick of the same run: the stats pass
      reads the embedding and src_pwr (a copy of HALF that many bytes reads and writes as much in total), the backward
      pass reads both and writes the gradient (a copy of the mean of the two);
  (4) Model.train_step at cfg 2 with the key at 0.1 against the key null: two models of the same seed.

    python tools/bench_dpcl.py [--rounds 7] [--reps 50] [--step-reps 20] [--no-train-step] [--out FILE]
'''
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SHAPES = (('cfg2_E20_C2', (32, 16512, 20, 2)), ('E40_C3', (32, 16512, 40, 3)))


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


def kernels_row(rounds, reps, tag, shape):
    import torch
    from danet_amd import _lib
    B, N, E, C = shape
    lib, st = _lib.load_dpcl(), _lib.stream()
    gen = torch.Generator(device='cuda').manual_seed(N % 1000 + E)
    embed = torch.randn(B, N, E, device='cuda', generator=gen)
    src_pwr = torch.rand(B, C, N, device='cuda', generator=gen)
    dembed = torch.empty_like(embed)
    nws = lib.danet_dpcl_workspace_bytes(B, N, E, C)
    ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    per_utt = torch.empty(B, dtype=torch.float64, device='cuda')
    main, dpcl, total = torch.ones(1, device='cuda'), torch.empty(1, device='cuda'), torch.empty(1, device='cuda')
    tables, cs = torch.empty(B, E, E + C, device='cuda'), torch.empty(B, C + 1, device='cuda')
    tiny = torch.ones(8, device='cuda')
    fwd_bytes = 4 * (embed.numel() + src_pwr.numel())
    bwd_bytes = fwd_bytes + 4 * embed.numel()
    pool = torch.empty(bwd_bytes // 4, device='cuda')                # copy source / destination of the yardsticks
    assert embed.data_ptr() % 16 == 0

    def stats():
        assert lib.danet_dpcl_stats(st, B, N, E, C, embed.data_ptr(), src_pwr.data_ptr(), ws.data_ptr(), nws) == 0

    def finalize():
        assert lib.danet_dpcl_finalize(st, B, N, E, C, ws.data_ptr(), nws, main.data_ptr(), 0.1, per_utt.data_ptr(),
                                       dpcl.data_ptr(), total.data_ptr(), tables.data_ptr(), cs.data_ptr()) == 0

    def bwd():
        assert lib.danet_dpcl_bwd(st, B, N, E, C, embed.data_ptr(), src_pwr.data_ptr(), tables.data_ptr(), cs.data_ptr(),
                                  main.data_ptr(), 0.1 / B, dembed.data_ptr()) == 0

    def floor():
        assert lib.danet_dpcl_bwd(st, 1, 1, 1, 1, tiny.data_ptr(), tiny.data_ptr(), tiny.data_ptr(), tiny.data_ptr(), None,
                                  1.0, tiny[4:].data_ptr()) == 0

    def copy_of(nbytes):
        n = nbytes // 8                                               # floats moved each way
        a, b = pool[:n], pool[n:2 * n]

        def fn():
            b.copy_(a)
        return fn

    fns = dict(launch_floor=floor, stats=stats, finalize=finalize, bwd=bwd, copy_fwd_bytes=copy_of(fwd_bytes),
               copy_bwd_bytes=copy_of(bwd_bytes))
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    r = dict(B=B, N=N, E=E, C=C, fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes, workspace_bytes=nws,
             chunks=lib.danet_dpcl_chunks(N), unit='us per call, back to back, C entry point')
    r.update({k: _summary(v) for k, v in t.items()})
    r['stats_GBps'] = round(fwd_bytes / r['stats']['median'] * 1e-3, 1)
    r['bwd_GBps'] = round(bwd_bytes / r['bwd']['median'] * 1e-3, 1)
    r['stats_over_copy'] = round(r['stats']['median'] / r['copy_fwd_bytes']['median'], 2)
    r['bwd_over_copy'] = round(r['bwd']['median'] / r['copy_bwd_bytes']['median'], 2)
    print('%s: stats %.1f us (%.0f GB/s, %.2f x its copy %.1f us), finalize %.1f us, bwd %.1f us (%.0f GB/s, %.2f x its '
          'copy %.1f us), floor %.1f us'
          % (tag, r['stats']['median'], r['stats_GBps'], r['stats_over_copy'], r['copy_fwd_bytes']['median'],
             r['finalize']['median'], r['bwd']['median'], r['bwd_GBps'], r['bwd_over_copy'],
             r['copy_bwd_bytes']['median'], r['launch_floor']['median']), file=sys.stderr)
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
    for tag, key in (('key_null', None), ('key_0.1', 0.1)):
        hparams.reset()
        hparams.load(dict(base, DPCL_WEIGHT=key))
        hparams.digest()
        models[tag] = Model('bench_dpcl', device='cuda:0', seed=7).build()
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
    for mdl in models.values():
        mdl.check_status()
    assert list(last['key_null']) == ['loss', 'SNR', 'LR'] and 'DPCL' in last['key_0.1']
    r = dict(config='cfg2', unit='us per train_step, back to back', key_null=_summary(t['key_null']),
             key_on=_summary(t['key_0.1']), dpcl=float(last['key_0.1']['DPCL']))
    r['added_us_per_step'] = round(r['key_on']['median'] - r['key_null']['median'], 2)
    r['added_percent'] = round(100.0 * r['added_us_per_step'] / r['key_null']['median'], 2)
    print('train_step: key null %.1f us (spread %.1f), key 0.1 %.1f us (spread %.1f): +%.1f us (%.2f %%)'
          % (r['key_null']['median'], r['key_null']['spread'], r['key_on']['median'], r['key_on']['spread'],
             r['added_us_per_step'], r['added_percent']), file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--step-reps', type=int, default=20)
    ap.add_argument('--no-train-step', action='store_true')
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_dpcl.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='deep-clustering auxiliary loss: stats, finalize, backward, copy yardsticks, train step; '
                        'interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, step_reps=args.step_reps, device=torch.cuda.get_device_name(0))
    res['kernels'] = {tag: kernels_row(args.rounds, args.reps, tag, shape) for tag, shape in SHAPES}
    if not args.no_train_step:
        res['train_step_cfg2'] = train_step_row(args.rounds, args.step_reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'dpcl_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
