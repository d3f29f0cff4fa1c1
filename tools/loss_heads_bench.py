"""Cost of the criterion block with every optional head, and of the training step, on this checkout and on the PARENT commit's
tree in ONE GPU session: one JSON line (and profiles/loss_heads_bench.json with --out).

The parent's tree, built, lies beside this one (--parent-tree):

    mkdir -p tools/build/parent_tree && git archive HEAD~1 | tar -x -C tools/build/parent_tree
    (cd tools/build/parent_tree && python -m offsetguided_amd.build)

  (a)/(b) criterion block: forward + backward through HeatMapsLoss and OffsetMapsLoss, both stacks, bs8, 128 x 128 maps (512 x 512
        crops), background + jitter + spread + keypoint-scale heads, --fused-losses true, between one pair of HIP timing events per
        iteration: median of TIMED iterations after WARM.  `all_heads`: focal-L2 heatmap and background, L1 jitter, laplace offsets
        (spread head), L1 scale.  `all_heads_vector`: the same with vector-L1 jitter and offsets.  `default`: no optional head, the
        default choices (both trees run the same two kernels).  The inputs are generated from a seed on the device, the same in
        both trees; the parent runs its torch formulation for every choice it has no kernel for.
  (c)   `python -m offsetguided_amd.train_dist --no-pretrain --bench` in each tree with default flags, and in this tree with
        --include-scale --include-jitter-offset --include-background: ms per step as the program reports it.
Child processes alternate (parent, this, parent, this, ...; --rounds of each); per arm the median over the rounds is reported
with the min .. max of the rounds, the spread of repeating the same command on the same code.

    python tools/loss_heads_bench.py --parent-tree tools/build/parent_tree [--out profiles/loss_heads_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, TIMED = 10, 30
CONFIGS = {
    'all_heads': dict(heads=True, hmp='focal_l2_loss', jit='offset_l1_loss', off='offset_laplace_loss'),
    'all_heads_vector': dict(heads=True, hmp='focal_l2_loss', jit='vector_l1_loss', off='vector_l1_loss'),
    'default': dict(heads=False, hmp='focal_l2_loss', jit='offset_l1_loss', off='offset_l1_loss'),
}
HEAD_FLAGS = ['--include-scale', '--include-jitter-offset', '--include-background']


def criterion_arm(tree):
    """Runs in a child process whose package is `tree`'s: {config: median ms of forward + backward through the criteria}."""
    sys.path.insert(0, tree)
    import torch
    from offsetguided_amd import _lib
    from offsetguided_amd.models import losses
    assert os.path.abspath(losses.__file__).startswith(os.path.abspath(tree) + os.sep), losses.__file__
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(7)
    n, h, w, kp, limbs = 8, 128, 128, 17, 19
    u = lambda c, lo, hi: torch.rand((n, c, h, w), generator=gen, device=dev) * (hi - lo) + lo  # noqa: E731

    def holes(pairs, undefined):       # both components of a vector, as the encoder writes them
        return (u(pairs, 0, 1) < undefined).repeat_interleave(2, dim=1)
    hm_gt = u(kp, 0, 1) * (u(kp, 0, 1) > 0.9)
    bg_gt = 1.0 - hm_gt.max(dim=1, keepdim=True)[0]
    jit_gt = u(2, -0.5, 0.5).masked_fill(holes(1, 0.9), float('inf'))
    off_gt = u(2 * limbs, -60, 60).masked_fill(holes(limbs, 0.9), float('inf'))
    sc_gt = u(kp, 1, 12).masked_fill(u(kp, 0, 1) < 0.9, float('nan'))
    ps, mask = u(2 * limbs, 20, 300), u(1, 0, 1) > 0.05
    pred = {k: [u(c, lo, hi).requires_grad_(True) for _ in range(2)]
            for k, (c, lo, hi) in dict(hm=(kp, -0.2, 1.1), bg=(1, -0.2, 1.1), jit=(2, -1, 1), off=(2 * limbs, -60, 60),
                                       spread=(limbs, -2, 3), scale=(kp, 0, 13)).items()}
    lambdas, none = [1.0, 1.0, 100.0, 100.0, 0.01], [[], []]
    out = {}
    for name, c in CONFIGS.items():
        crit = losses.lossfuncs_factory(['hmp', 'omp'], 2, [1, 1], c['hmp'], c['jit'], c['off'], 'scale_l1_loss', False, fused=True)
        on = c['heads']

        def block():
            for ps_ in pred.values():      # a fresh gradient per iteration, as in a training step
                for t in ps_:
                    t.grad = None
            parts = list(crit[0]((pred['hm'], pred['bg'] if on else none, pred['jit'] if on else none), hm_gt,
                                 bg_gt if on else None, jit_gt if on else None, mask))
            parts += list(crit[1]((pred['off'], pred['spread'] if on else none, pred['scale'] if on else none), off_gt,
                                  sc_gt if on else None, ps, mask))
            loss = sum(lam * l for lam, l in zip(lambdas, parts))
            loss.backward()
            return loss
        for _ in range(WARM):
            block()
        torch.cuda.synchronize(dev)
        st, pairs = torch.cuda.current_stream(dev), []
        for _ in range(TIMED):
            a, b = _lib.TimingEvent(), _lib.TimingEvent()
            a.record(st)
            loss = block()
            b.record(st)
            pairs.append((a, b))
        torch.cuda.synchronize(dev)
        out[name] = {'ms': round(statistics.median(a.elapsed_time(b) for a, b in pairs), 4), 'loss': float(loss)}
    print('ARM ' + json.dumps(out))


def child(tree, argv, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'OG_DECODER_LIB')}
    env['PYTHONPATH'] = tree
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, cwd=tree, env=env)
    if r.returncode != 0:
        raise RuntimeError(f'{argv} in {tree} failed ({r.returncode}):\n{r.stderr[-3000:]}')
    return r.stdout


def spread(values):
    return [round(statistics.median(values), 4), round(min(values), 4), round(max(values), 4)]


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--parent-tree', default=os.path.join(ROOT, 'tools', 'build', 'parent_tree'))
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--train-rounds', type=int, default=2)
    p.add_argument('--bench-steps', type=int, default=20)
    p.add_argument('--out', default=None)
    p.add_argument('--arm', default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.arm:
        return criterion_arm(a.arm)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('loss_heads_bench: no HIP device; a timing needs the GPU')
    trees = {'parent': os.path.abspath(a.parent_tree), 'this': ROOT}
    if not os.path.exists(os.path.join(trees['parent'], 'offsetguided_amd', 'libog_decoder.so')):
        raise SystemExit(f"{trees['parent']}: the parent commit's tree with its library built is needed (see the module docstring)")
    crit = {k: {c: [] for c in CONFIGS} for k in trees}
    losses_seen = {k: {} for k in trees}
    train = {'parent_default': [], 'this_default': [], 'this_scale_jitter_background': []}
    workload = {}
    device = torch.cuda.get_device_name(0)

    def report():
        """The result so far; written to --out after every child, so a run that is cut short leaves what it measured."""
        result = {
            'what': 'criterion block (forward + backward through the criteria, both stacks, bs8, 128x128 maps) and train_dist '
                    '--bench (512x512 crops, bs8, one GPU), this tree and the parent commit in one session; [median, min, max] '
                    'over the rounds',
            'device': device, 'warm': WARM, 'timed': TIMED, 'rounds': a.rounds, 'train_rounds': a.train_rounds,
            'bench_steps': a.bench_steps, 'configs': CONFIGS,
            'criterion_ms': {k: {c: spread(v) for c, v in d.items() if v} for k, d in crit.items()},
            'criterion_ms_rounds': crit, 'criterion_loss_value': losses_seen,
            'train_step_ms': {k: spread(v) for k, v in train.items() if v}, 'train_step_ms_rounds': train,
            'train_workload': workload}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps(result, indent=1) + '\n')
        return result

    for _ in range(a.rounds):
        for k, tree in trees.items():
            line = [l for l in child(tree, [os.path.abspath(__file__), '--arm', tree], 600).splitlines() if l.startswith('ARM ')][-1]
            for c, v in json.loads(line[4:]).items():
                crit[k][c].append(v['ms'])
                losses_seen[k][c] = v['loss']
            report()
    bench = ['-m', 'offsetguided_amd.train_dist', '--no-pretrain', '--bench', '--bench-steps', str(a.bench_steps), '--bench-warmup', '5']
    for _ in range(a.train_rounds):
        for name, tree, extra in (('parent_default', trees['parent'], []), ('this_default', ROOT, []),
                                  ('this_scale_jitter_background', ROOT, HEAD_FLAGS)):
            d = json.loads([l for l in child(tree, bench + extra, 1500).splitlines() if l.startswith('{')][-1])
            train[name].append(d['ms_per_step'])
            workload[name] = d['config']['workload']
            report()
    print(json.dumps(report()))


if __name__ == '__main__':
    main()
