#!/usr/bin/env python3
"""What the reconstruction's side stream costs, over EVERY mid-run step of a rocprofv3 kernel trace (dev tool; tools/trace.py prints one step).
   tools/tlgaps.py <dir> [skip = 4]  -- per step: the period, the gap behind fwd_cols (the fork), the gap in front of kspec (the join) and the
   durations of the kernels on either side of them; then mean, median and min-max over the steps.  The first `skip` steps and the last four
   (the profiled roofline pass, if any, and the run's end) are left out."""
import csv, glob, statistics, sys
path = sys.argv[1]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 4
f = glob.glob(path + '/**/*kernel_trace.csv', recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if 'aefft' in r['Kernel_Name']]
rows.sort(key=lambda r: int(r['Start_Timestamp']))
idx = [i for i, r in enumerate(rows) if 'r2c_rows' in r['Kernel_Name']]
NAMES = ['r2c_rows', 'fwd_cols', 'msgrad', 'inv_cols', 'kgrad', 'c2r_rows', 'wgrad', 'kspec', 'tail']
cols = ['period', 'gap_fork', 'gap_join'] + NAMES
steps = []
for k in range(skip, len(idx) - 4):
    seg = rows[idx[k]:idx[k + 1]]
    by = {}
    for r in seg:
        for n in NAMES:
            if n + '_' in r['Kernel_Name'] and n not in by:
                by[n] = (int(r['Start_Timestamp']), int(r['End_Timestamp']))
    if len(by) != len(NAMES):
        continue
    d = {n: (by[n][1] - by[n][0]) / 1e3 for n in NAMES}
    d['period'] = (int(rows[idx[k + 1]]['Start_Timestamp']) - by['r2c_rows'][0]) / 1e3
    d['gap_fork'] = (by['msgrad'][0] - by['fwd_cols'][1]) / 1e3
    d['gap_join'] = (by['kspec'][0] - by['wgrad'][1]) / 1e3
    steps.append(d)
print(f"{len(steps)} steps of {len(idx)} (us)")
print(' '.join(f"{c:>9}" for c in ['stat'] + cols))
for name, fn in (('mean', statistics.fmean), ('median', statistics.median), ('min', min), ('max', max)):
    print(' '.join([f"{name:>9}"] + [f"{fn([s[c] for s in steps]):9.1f}" for c in cols]))
