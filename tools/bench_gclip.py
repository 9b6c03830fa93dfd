'''
What global-norm gradient clipping (GRAD_CLIP_NORM) costs, measured in ONE process on one box with INTERLEAVED
blocks; prints one JSON line and writes it to profiles/gclip_bench.json.  Every row carries the per-block figures,
their median and the block-to-block spread (max - min): a difference inside the spread counts as equal.

  (a) danet_gclip_sumsq alone at n = 6 904 920 (cfg 2) and 35 615 000 (cfg 4h600), aligned: --reps back-to-back
      calls between two events per block, us per call and GB/s, next to the launch floor of the same run (the same
      entry point at n = 1); then ONE call between two events of its own right after a kernel that wrote the
      gradient, and after a 1 GiB fill has swept the caches, next to the floor bracketed the same way;
  (b) danet_gclip_adam_step against danet_adam_clip_step at the same n, back to back: the difference is what the
      prologue costs.  With --variants, the same two rows for the variant libraries `--build-variants` made
      (DANET_GCLIP_MAX_PARTIALS = 256 and 512 beside the shipped 1024): the measurement behind that choice;
  (c) Model.train_step at cfg 2 with the key at a value that clips against the key null: two models of the same
      seed.  BAR, same run: added time <= two launch floors + the back-to-back time of danet_gclip_sumsq from (a).

    python tools/bench_gclip.py --build-variants          (no GPU needed: compiles the variant libraries)
    python tools/bench_gclip.py [--rounds 7] [--reps 50] [--step-reps 20] [--variants] [--out FILE]
'''
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SIZES = (('cfg2', 6904920), ('cfg4h600', 35615000))
VARIANTS = (256, 512)
HYPER = (2.5e-3, 0.9, 0.999, 1e-8, 100.0)


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


def _bracketed(before, fn, reps):
    '''us per call of ONE fn() between two events of its own, each right behind before()'''
    import torch
    evs = []
    for _ in range(reps):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in evs) * 1e3 / reps


def _variant_path(P):
    import importlib
    build = importlib.import_module('danet-tensorflow_amd._build')
    return os.path.join(build.CSRC, 'libdanet_gclip_hip_p%d.so' % P)


def build_variants():
    import importlib
    build = importlib.import_module('danet-tensorflow_amd._build')
    for P in VARIANTS:
        bdir = os.path.join(build.GCLIP.src_dir, 'build_p%d' % P)
        res = build._compile_all(build.GCLIP.src_dir, bdir, True, 0.0, ['-DDANET_GCLIP_MAX_PARTIALS=%d' % P])
        build._link([o for o, _ in res], _variant_path(P), build.GCLIP.src_dir)
        print(_variant_path(P))


def _bind(path):
    from danet_amd import _lib
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in _lib.GCLIP_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def kernels_row(rounds, reps, tag, n, variants):
    import torch
    from danet_amd import _lib
    core, st = _lib.load(), _lib.stream()
    libs = {1024: _lib.load_gclip()}
    for P in variants:
        libs[P] = _bind(_variant_path(P))
    gen = torch.Generator(device='cuda').manual_seed(n % 1000)
    grad = torch.randn(n, device='cuda', generator=gen) * 1e-2
    src = grad.clone()
    theta, m, v = torch.randn(n, device='cuda', generator=gen), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    sweep = torch.empty(1 << 28, device='cuda')                       # 1 GiB: four times the last-level cache
    parts = {P: torch.zeros(lib.danet_gclip_partials(n), dtype=torch.float64, device='cuda') for P, lib in libs.items()}
    one = torch.zeros(1, dtype=torch.float64, device='cuda')
    out = torch.zeros(2, dtype=torch.float64, device='cuda')
    assert grad.data_ptr() % 16 == 0

    def sumsq(P):
        def fn():
            assert libs[P].danet_gclip_sumsq(st, n, grad.data_ptr(), parts[P].data_ptr(), parts[P].numel()) == 0
        return fn

    def fused(P):
        def fn():
            assert libs[P].danet_gclip_adam_step(st, n, theta.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                 *HYPER, 1.0, 0, 1e30, parts[P].data_ptr(), parts[P].numel(),
                                                 out.data_ptr()) == 0
        return fn

    def core_step():
        assert core.danet_adam_clip_step(st, n, theta.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), *HYPER,
                                         1.0, 0) == 0

    def floor():
        assert libs[1024].danet_gclip_sumsq(st, 1, grad.data_ptr(), one.data_ptr(), 1) == 0

    fns = dict(launch_floor=floor, core_adam_step=core_step)
    for P in libs:
        suffix = '' if P == 1024 else '_p%d' % P
        fns['sumsq' + suffix] = sumsq(P)
        fns['fused_adam_step' + suffix] = fused(P)
    for _ in range(5):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    r = dict(n=n, bytes=4 * n, partials={str(P): p.numel() for P, p in parts.items()},
             unit='us per call, back to back, C entry point')
    r.update({k: _summary(val) for k, val in t.items()})
    r['sumsq_GBps'] = round(4 * n / r['sumsq']['median'] * 1e-3, 1)
    r['prologue_us'] = round(r['fused_adam_step']['median'] - r['core_adam_step']['median'], 3)
    # one call between two events of its own: behind a kernel that wrote the gradient, and behind a cache sweep
    br = {k: [] for k in ('floor_after_write', 'sumsq_after_write', 'floor_after_sweep', 'sumsq_after_sweep')}
    few = max(4, reps // 5)
    for _ in range(rounds):
        br['floor_after_write'].append(_bracketed(lambda: grad.copy_(src), floor, few))
        br['sumsq_after_write'].append(_bracketed(lambda: grad.copy_(src), sumsq(1024), few))
        br['floor_after_sweep'].append(_bracketed(lambda: sweep.fill_(0.0), floor, few))
        br['sumsq_after_sweep'].append(_bracketed(lambda: sweep.fill_(0.0), sumsq(1024), few))
    r['bracketed'] = dict(unit='us, ONE call between two events of its own', **{k: _summary(val) for k, val in br.items()})
    r['bracketed']['after_write_GBps'] = round(4 * n / r['bracketed']['sumsq_after_write']['median'] * 1e-3, 1)
    r['bracketed']['after_sweep_GBps'] = round(4 * n / r['bracketed']['sumsq_after_sweep']['median'] * 1e-3, 1)
    print('%s n %d: sumsq %.1f us (%.0f GB/s), floor %.1f us; after a write %.1f us, after a sweep %.1f us (floor %.1f '
          '/ %.1f); fused %.1f us vs core %.1f us: prologue %+.1f us'
          % (tag, n, r['sumsq']['median'], r['sumsq_GBps'], r['launch_floor']['median'],
             r['bracketed']['sumsq_after_write']['median'], r['bracketed']['sumsq_after_sweep']['median'],
             r['bracketed']['floor_after_write']['median'], r['bracketed']['floor_after_sweep']['median'],
             r['fused_adam_step']['median'], r['core_adam_step']['median'], r['prologue_us']), file=sys.stderr)
    return r


def train_step_row(rounds, reps, kernels):
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
    for tag, key in (('key_null', None), ('key_clips', 1e-3)):
        hparams.reset()
        hparams.load(dict(base, GRAD_CLIP_NORM=key))
        hparams.digest()
        models[tag] = Model('bench_gclip', device='cuda:0', seed=7).build()
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
    n = models['key_clips']._flat_grad.numel()
    assert float(last['key_clips']['clip_coef']) < 1.0 and list(last['key_null']) == ['loss', 'SNR', 'LR']
    r = dict(config='cfg2', parameters=n, unit='us per train_step, back to back', key_null=_summary(t['key_null']),
             key_clips=_summary(t['key_clips']), grad_norm=float(last['key_clips']['grad_norm']),
             clip_coef=float(last['key_clips']['clip_coef']))
    r['added_us_per_step'] = round(r['key_clips']['median'] - r['key_null']['median'], 2)
    ref = kernels.get('cfg2')
    if ref is not None and ref['n'] == n:
        r['bar_us'] = round(2 * ref['launch_floor']['median'] + ref['sumsq']['median'], 2)
        r['bar'] = 'two launch floors + the back-to-back time of danet_gclip_sumsq, same run'
        r['bar_met'] = bool(r['added_us_per_step'] <= r['bar_us'])
    print('train_step: key null %.1f us (spread %.1f), key clips %.1f us (spread %.1f): +%.1f us, bar %s us'
          % (r['key_null']['median'], r['key_null']['spread'], r['key_clips']['median'], r['key_clips']['spread'],
             r['added_us_per_step'], r.get('bar_us')), file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--step-reps', type=int, default=20)
    ap.add_argument('--build-variants', action='store_true', help='compile the variant libraries and exit')
    ap.add_argument('--variants', action='store_true', help='also time the variant libraries')
    ap.add_argument('--no-train-step', action='store_true')
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_gclip.py measures on the GPU'
    torch.cuda.set_device(0)
    variants = VARIANTS if args.variants else ()
    res = dict(workload='global-norm gradient clipping: sum of squares, fused clip + Adam step, train step; interleaved '
                        'blocks in one process',
               rounds=args.rounds, reps=args.reps, step_reps=args.step_reps, device=torch.cuda.get_device_name(0))
    res['ab_kernels'] = {tag: kernels_row(args.rounds, args.reps, tag, n, variants) for tag, n in SIZES}
    if not args.no_train_step:
        res['c_train_step_cfg2'] = train_step_row(args.rounds, args.step_reps, res['ab_kernels'])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'gclip_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
