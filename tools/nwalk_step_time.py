"""Step time of the flagship benchmark with the N-inner walk of the short-K fused bottleneck tails off / on (SIMCLR_IGEMM_NWALK=0 / 1,
csrc/igemm_nwalk.h), everything in ONE call on one machine:
    python tools/nwalk_step_time.py [--parent_lib libsimclr_hip_parent.so] [--pairs 3] [--out nwalk_step_time_results.json]
Every measurement is a fresh `bench.py --gpus 1` child process with the benchmark's default steps / warm-up: the parent commit's
library once (SIMCLR_HIP_LIB; it ignores the switch), then `pairs` interleaved (switch 0, switch 1) pairs of this build.
The acceptance rule is evaluated here: every pair favours switch 1, and the mean gain is at least three times the spread (max - min)
of the switch-0 repeats."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(env, timeout=900):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'], env=e, capture_output=True, text=True,
                       timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('bench.py failed with exit status %d: nothing more is started' % r.returncode)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    return json.loads(lines[-1])


def brief(line):
    keep = ('ms_per_step', 'value', 'unit', 'steps', 'warmup', 'dtype', 'f32_matmul', 'step_ms', 'north_star_met', 'parity')
    return {k: line[k] for k in keep if k in line}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent_lib', default=None, help="the parent commit's libsimclr_hip.so")
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--out', default='nwalk_step_time_results.json')
    args = ap.parse_args()
    res = dict(what='bench.py --gpus 1 with its default steps / warm-up (fp32 storage, f16x3_3), fresh process per measurement, one GPU call')

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    if args.parent_lib:
        res['parent_commit'] = brief(bench(dict(SIMCLR_HIP_LIB=os.path.abspath(args.parent_lib))))
        print('parent commit: %.3f ms' % res['parent_commit']['ms_per_step'], flush=True)
        save()
    pairs = []
    for i in range(args.pairs):
        a = brief(bench(dict(SIMCLR_IGEMM_NWALK='0')))
        b = brief(bench(dict(SIMCLR_IGEMM_NWALK='1')))
        pairs.append(dict(pair=i + 1, switch0=a, switch1=b, gain_ms=round(a['ms_per_step'] - b['ms_per_step'], 3)))
        print('pair %d: switch 0 %.3f ms, switch 1 %.3f ms, gain %.3f ms' % (i + 1, a['ms_per_step'], b['ms_per_step'], pairs[-1]['gain_ms']), flush=True)
        res['pairs'] = pairs
        save()
    s0 = [p['switch0']['ms_per_step'] for p in pairs]
    s1 = [p['switch1']['ms_per_step'] for p in pairs]
    res['switch0_ms'], res['switch1_ms'] = s0, s1
    res['switch0_spread_ms'] = round(max(s0) - min(s0), 3)
    res['mean_gain_ms'] = round(sum(s0) / len(s0) - sum(s1) / len(s1), 3)
    res['every_pair_favours_switch1'] = all(p['gain_ms'] > 0 for p in pairs)
    res['accepted_by_rule'] = bool(res['every_pair_favours_switch1'] and res['mean_gain_ms'] >= 3 * res['switch0_spread_ms'])
    # (a lean bench.py run does not measure parity: north_star_met is null there and comes from a `bench.py --full` run instead)
    met = [p[k].get('north_star_met') for p in pairs for k in ('switch0', 'switch1')]
    res['north_star_met'] = None if any(m is None for m in met) else all(met)
    if args.parent_lib:
        res['mean_gain_vs_parent_ms'] = round(res['parent_commit']['ms_per_step'] - sum(s1) / len(s1), 3)
    save()
    print(json.dumps({k: res[k] for k in ('switch0_ms', 'switch1_ms', 'switch0_spread_ms', 'mean_gain_ms', 'every_pair_favours_switch1',
                                          'accepted_by_rule', 'north_star_met') if k in res}))


if __name__ == '__main__':
    main()
