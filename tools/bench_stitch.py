'''
What chunked inference (INFER_CHUNK_LEN) costs, measured in ONE process on one box with INTERLEAVED blocks; prints one
JSON line and writes it to profiles/stitch_bench.json.  Every row carries the per-block figures, their median and the
block-to-block spread (max - min): a difference inside the spread counts as equal.

  (1) danet_stitch_affinity, danet_stitch_assign and danet_stitch_merge alone through the C ABI at a 60 s / 8 kHz
      recording, (T, L, V, C, F) = (7500, 512, 128, 2, 129): --reps back-to-back calls between two events per block,
      us per call, next to the launch floor of the same run (danet_stitch_merge at T = 3, L = 2, V = C = F = 1);
  (2) Model.infer of the same recording (cfg 2's network: 3 x BiLSTM 300, FFT 256 / 64, batch 1) with the keys set
      (infer_long: 20 chunks in groups of 16) against the key null (one sequence of 7500 frames): two models of the
      same seed, ms per call.

    python tools/bench_stitch.py [--rounds 7] [--reps 50] [--infer-reps 3] [--no-infer] [--out FILE]
'''
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SHAPE = (7500, 512, 128, 2, 129)


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


def kernels_row(rounds, reps):
    import torch
    from danet_amd import _lib, ops
    T, L, V, C, F = SHAPE
    lib, st = _lib.load_stitch(), _lib.stream()
    n = lib.danet_stitch_chunks(T, L, V)
    starts = ops.stitch_plan(T, L, V)
    gen = torch.Generator(device='cuda').manual_seed(T)
    mags = torch.rand(n, C, L, F, device='cuda', generator=gen)
    th = torch.rand(n, L, F, device='cuda', generator=gen) * 6.28
    phasor = torch.stack([torch.cos(th), torch.sin(th)], dim=-1).contiguous()
    fade = ops.stitch_fade(V, mags.device)
    nws = lib.danet_stitch_workspace_bytes(T, L, V, C, F)
    ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    S = torch.empty(n - 1, C, C, dtype=torch.float64, device='cuda')
    perm = torch.empty(n, C, dtype=torch.int32, device='cuda')
    out = torch.empty(C, T, F, 2, device='cuda')
    tiny = torch.ones(64, device='cuda')
    tiny_perm = torch.zeros(8, dtype=torch.int32, device='cuda')
    overlap_frames = sum(a + L - b for a, b in zip(starts, starts[1:]))
    affinity_bytes = 2 * C * overlap_frames * F * 4                    # both factors of every overlap, once
    merge_bytes = C * T * F * 4 + T * F * 8 + C * T * F * 8           # one source, the phasor, the output
    assert mags.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0

    def affinity():
        assert lib.danet_stitch_affinity(st, T, L, V, C, F, mags.data_ptr(), ws.data_ptr(), nws) == 0

    def assign():
        assert lib.danet_stitch_assign(st, T, L, V, C, F, ws.data_ptr(), nws, S.data_ptr(), perm.data_ptr()) == 0

    def merge():
        assert lib.danet_stitch_merge(st, T, L, V, C, F, mags.data_ptr(), phasor.data_ptr(), fade.data_ptr(),
                                      perm.data_ptr(), out.data_ptr()) == 0

    def floor():
        assert lib.danet_stitch_merge(st, 3, 2, 1, 1, 1, tiny.data_ptr(), tiny[8:].data_ptr(), tiny[32:].data_ptr(),
                                      tiny_perm.data_ptr(), tiny[40:].data_ptr()) == 0

    fns = dict(launch_floor=floor, affinity=affinity, assign=assign, merge=merge)
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    r = dict(T=T, L=L, V=V, C=C, F=F, chunks=n, workspace_bytes=nws, affinity_bytes=affinity_bytes,
             merge_bytes=merge_bytes, unit='us per call, back to back, C entry point')
    r.update({k: _summary(v) for k, v in t.items()})
    r['affinity_GBps'] = round(affinity_bytes / r['affinity']['median'] * 1e-3, 1)
    r['merge_GBps'] = round(merge_bytes / r['merge']['median'] * 1e-3, 1)
    print('affinity %.1f us (%.0f GB/s), assign %.1f us, merge %.1f us (%.0f GB/s), floor %.1f us'
          % (r['affinity']['median'], r['affinity_GBps'], r['assign']['median'], r['merge']['median'], r['merge_GBps'],
             r['launch_floor']['median']), file=sys.stderr)
    return r


def infer_row(rounds, reps):
    import numpy as np
    import torch
    import bench
    from danet_amd.hparams import hparams
    from danet_amd.model import Model
    T, L, V, _C, F = SHAPE
    cfg = bench.CONFIGS['cfg2']
    base = dict(cfg['hp'], BATCH_SIZE=1, NUM_LSTM_LAYERS=cfg['layers'], LSTM_HDIM=cfg['hdim'],
                ENCODER_TYPE='bilstm-orig', OPTIMIZER_TYPE='adam')
    rng = np.random.RandomState(1)
    x = torch.from_numpy(((rng.randn(1, T, F) + 1j * rng.randn(1, T, F)) * 3).astype(np.complex64)).cuda()
    models = {}
    for tag, keys in (('key_null', {}), ('chunked', dict(INFER_CHUNK_LEN=L, INFER_CHUNK_OVERLAP=V))):
        hparams.reset()
        hparams.load(dict(base, **keys))
        hparams.digest()
        models[tag] = Model('bench_stitch', device='cuda:0', seed=7).build()
    peak = {}

    def call(tag):
        def fn():
            models[tag].infer(x)
        return fn
    for tag in models:
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        for _ in range(2):
            call(tag)()
        torch.cuda.synchronize()
        peak[tag] = torch.cuda.max_memory_allocated() - before
    t = {tag: [] for tag in models}
    for _ in range(rounds):
        for tag in models:
            t[tag].append(_timed_launches(call(tag), reps) * 1e-3)
    for mdl in models.values():
        mdl.check_status()
    r = dict(config='cfg2 network, batch 1, T = %d' % T, unit='ms per Model.infer, back to back',
             key_null=_summary(t['key_null']), chunked=_summary(t['chunked']),
             infer_chunk=list(models['chunked'].infer_chunk), peak_bytes_above_start=peak)
    r['chunked_over_key_null'] = round(r['chunked']['median'] / r['key_null']['median'], 3)
    print('infer: key null %.2f ms (spread %.2f), chunked %.2f ms (spread %.2f): x %.3f; peak bytes %s'
          % (r['key_null']['median'], r['key_null']['spread'], r['chunked']['median'], r['chunked']['spread'],
             r['chunked_over_key_null'], peak), file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--infer-reps', type=int, default=3)
    ap.add_argument('--no-infer', action='store_true')
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_stitch.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='chunked inference: affinity, assign, merge, launch floor, Model.infer chunked against one '
                        'sequence; interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, infer_reps=args.infer_reps, device=torch.cuda.get_device_name(0))
    res['kernels'] = kernels_row(args.rounds, args.reps)

    def write():
        line = json.dumps(res)
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        for path in [os.path.join(ROOT, 'profiles', 'stitch_bench.json')] + ([args.out] if args.out else []):
            with open(path, 'w') as f:
                f.write(line + '\n')
        return line
    write()                      # the kernel rows are kept even if the recording does not fit the device below
    if not args.no_infer:
        res['infer_60s_8kHz'] = infer_row(args.rounds, args.infer_reps)
    print(write())


if __name__ == '__main__':
    main()
