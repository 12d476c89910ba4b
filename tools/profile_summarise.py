#!/usr/bin/env python
"""Turn the rocprofv3 CSVs of tools/profile_round.sh into the small, committed evidence files under
profiles/: <tag>_kernel_stats.csv (per-kernel calls / average), <tag>_pmc_traffic.json (HBM bytes
per launch of the streaming kernels) and <tag>_summary.md."""
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def find(d, pat):
    fs = glob.glob(os.path.join(d, '**', pat), recursive=True)
    return max(fs, key=os.path.getmtime) if fs else None      # gpurun merges: keep the newest run's file


def main():
    out_dir, tag = sys.argv[1], sys.argv[2]
    bench_args = ' '.join(sys.argv[3:])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prof = os.path.join(root, 'profiles')
    os.makedirs(prof, exist_ok=True)
    stats = find(os.path.join(out_dir, 'stats'), '*kernel_stats.csv')
    rows = list(csv.DictReader(open(stats)))
    with open(os.path.join(prof, tag + '_kernel_stats.csv'), 'w') as f:
        w = csv.writer(f)
        w.writerow(['Name', 'Calls', 'TotalDurationNs', 'AverageNs', 'Percentage'])
        for r in rows:
            w.writerow([r['Name'], r['Calls'], r['TotalDurationNs'], r['AverageNs'], r['Percentage']])
    log = os.path.join(out_dir, 'bench_under_rocprof.log')
    if not os.path.exists(log):
        log = os.path.join(out_dir, 'bench.log')
    bench_line = [l for l in open(log).read().splitlines()
                  if l.startswith('{"metric"')][-1]
    open(os.path.join(prof, tag + '_bench_under_rocprof.log'), 'w').write(bench_line + '\n')
    bench = json.loads(bench_line)

    def pmc(sub, counter):
        f = find(os.path.join(out_dir, sub), '*counter_collection.csv')
        acc = defaultdict(list)
        for r in csv.DictReader(open(f)):
            if r['Counter_Name'] == counter:
                acc[r['Kernel_Name']].append(float(r['Counter_Value']))
        return {k: sum(v) / len(v) for k, v in acc.items() if len(v) >= 10}
    fetch, write = pmc('pmc_fetch', 'FETCH_SIZE'), pmc('pmc_write', 'WRITE_SIZE')
    traffic = {'_how': 'rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE, two separate passes over '
                       '`python bench.py --steps 30 --warmup 5 --no-cpu-baseline --no-extra ' + bench_args + '`; per-dispatch '
                       'averages. Units: KB (x1024). gfx950 correction (MI355X_MICROARCH.md, HBM): FETCH_SIZE counts '
                       '64 B per 128-B request of a wide coalesced stream -> doubled; the forward pooling pass '
                       '(reads exactly X) is the calibration row.'}
    cfg = bench['config']['workload']
    for name in fetch:
        if 'pool_fwd' in name or 'bwd_main' in name:
            short = name.split('(')[0].replace('void apa::', '')
            traffic[short] = {'FETCH_SIZE_KB_raw': round(fetch[name], 1), 'WRITE_SIZE_KB': round(write.get(name, 0.0), 1),
                              'hbm_bytes_per_launch': int((2 * fetch[name] + write.get(name, 0.0)) * 1024),
                              'workload': cfg}
    json.dump(traffic, open(os.path.join(prof, tag + '_pmc_traffic.json'), 'w'), indent=1)

    per_step = [r for r in rows if int(r['Calls']) >= 200 and 'apa::' in r['Name']]
    with open(os.path.join(prof, tag + '_summary.md'), 'w') as f:
        f.write('# {} rocprofv3 summary (MI355X, gfx950)\n\n'.format(tag))
        cmd = 'python bench.py --steps 200 --warmup 20 --full --no-cpu-baseline --no-extra ' + bench_args
        if os.path.exists(os.path.join(out_dir, 'cmd.txt')):
            cmd = open(os.path.join(out_dir, 'cmd.txt')).read().strip()
        f.write('Command (inside gpurun): `rocprofv3 --kernel-trace --stats --output-format csv -- {}`\n\n'
                '(workload: {})\n\n'.format(cmd, cfg))
        f.write('bench line under the profiler: {} img/s, {:.2f} us/step\n\n'.format(bench['value'], bench['ms_per_step'] * 1e3))
        f.write('| kernel | calls | avg us | % |\n|---|---|---|---|\n')
        for r in per_step:
            f.write('| `{}` | {} | {:.2f} | {} |\n'.format(r['Name'].replace('(anonymous namespace)::', '').split('(')[0], r['Calls'], float(r['AverageNs']) / 1e3, r['Percentage']))
        rl, rf = bench.get('roofline', {}), bench.get('roofline_fwd', {})
        f.write('\nCross-check of bench.py\'s own kernel timer (hipExtLaunchKernel start/stop events) against the '
                'rocprofv3 averages above, same run:\n\n| kernel | bench.py avg us | rocprofv3 avg us | ratio |\n|---|---|---|---|\n')
        for r in per_step:
            for tag_, blk in (('bwd_main', rl), ('pool_fwd', rf)):
                if tag_ in r['Name'] and blk.get('kernel_avg_us'):
                    ra = float(r['AverageNs']) / 1e3
                    f.write('| `{}` | {:.2f} | {:.2f} | {:.3f} |\n'.format(blk['kernel'], blk['kernel_avg_us'], ra,
                                                                         blk['kernel_avg_us'] / ra))
        if rl:
            f.write('\nroofline (bench line): {} GB/s = {} of {} GB/s on {} B per launch\n'.format(
                rl.get('achieved'), rl.get('frac'), rl.get('peak'), rl.get('alg_bytes_per_launch')))
        f.write('\nrocprofv3 kernel durations include ~1.5 us of dispatch overhead per kernel (an empty kernel '
                'reads 1.5 us min / 4.6 us median under the profiler, measured in round 2), so the small kernels look '
                'bigger here than their marginal cost in the un-profiled step.\n\n')
        f.write('HBM traffic per launch (PMC, separate passes): see `{}_pmc_traffic.json`\n'.format(tag))
        for k, v in traffic.items():
            if k != '_how':
                f.write('- `{}`: {:.2f} MB\n'.format(k, v['hbm_bytes_per_launch'] / 1e6))
    print(open(os.path.join(prof, tag + '_summary.md')).read())


if __name__ == '__main__':
    main()
