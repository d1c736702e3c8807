"""Timeline of the launch groups in a rocprofv3 --kernel-trace of bench.py: every kernel of the timed region with queue, start,
end and whether it overlaps another queue's kernel, then ONE line that splits the region into forward, preparation,
backtrace and idle time (profiles/r03_backtrace_overlap.txt has the shape).

    rocprofv3 --kernel-trace -d DIR -o x --output-format csv -- python bench.py --steps 16
    python tools/overlap_report.py DIR/.../x_kernel_trace.csv --groups 2 [--title TEXT]

A launch group starts with nonfinite::matrix_kernel (the first kernel run_resident enqueues) and holds what its queue runs
up to the next one.  bench.py decodes one warm-up group first; the `--groups` groups behind it are the timed region (the
groups bench.py profiles afterwards are listed with --all).  Times in ms from the region's first kernel.
"""
import argparse
import csv
import re

PHASES = [('forward', r'resident_forward_kernel'),
          ('backtrace', r'group_backtrace|group_segment|group_stitch|nonfinite::repair_kernel'),
          ('preparation', r'nonfinite::matrix_kernel|sort_rows_kernel|arrange_blocks_kernel|transpose_kernel|order_\w+_kernel|'
                          r'absent_kernel')]


def phase_of(name):
    for phase, pattern in PHASES:
        if re.search(pattern, name):
            return phase
    return None


def short(name):
    name = re.sub(r'^void ', '', name)
    return re.sub(r'\((?:[^()]|\([^()]*\))*\)( \[clone .*\])?$', '', name)


def read(path):
    rows = []
    with open(path, newline='') as f:
        for r in csv.DictReader(f):
            name = r.get('Kernel_Name') or r.get('Name')
            grid = 1
            for axis in 'XYZ':
                grid *= int(r.get(f'Grid_Size_{axis}') or 1)
            rows.append({'name': name, 'queue': r.get('Queue_Id', '?'), 'start': int(r['Start_Timestamp']),
                         'end': int(r['End_Timestamp']), 'grid': grid, 'phase': phase_of(name)})
    rows.sort(key=lambda k: (k['start'], k['end']))
    return rows


def groups_of(rows):
    """Kernels of the phases above, each tagged with the number of its launch group (by start of the group's first kernel)."""
    open_group = {}          # queue -> group number
    count = 0
    kept = []
    for k in rows:
        if k['phase'] is None:
            continue
        if 'nonfinite::matrix_kernel' in k['name']:
            open_group[k['queue']] = count
            count += 1
        if k['queue'] in open_group:
            kept.append(dict(k, group=open_group[k['queue']]))
    return kept, count


def covered(intervals):
    """Total length of the union of [start, end) intervals, and the merged intervals."""
    merged = []
    for a, b in sorted(intervals):
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    return sum(b - a for a, b in merged), merged


def outside(intervals, mask):
    """Length of the union of `intervals` that lies outside the merged intervals `mask`."""
    total, merged = covered(intervals)
    for a, b in merged:
        for c, d in mask:
            total -= max(0, min(b, d) - max(a, c))
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('trace')
    ap.add_argument('--groups', type=int, default=2, help='timed launch groups (steps / 8)')
    ap.add_argument('--all', action='store_true', help='list the warm-up group and the profiled groups too')
    ap.add_argument('--title', default=None)
    ap.add_argument('--brief', action='store_true', help='list only kernels of at least 20 us')
    args = ap.parse_args()
    kernels, count = groups_of(read(args.trace))
    if count < args.groups + 1:
        raise SystemExit(f'{count} launch groups in the trace, {args.groups + 1} needed (one warm-up group first)')
    timed = [k for k in kernels if 1 <= k['group'] <= args.groups]
    t0, t1 = min(k['start'] for k in timed), max(k['end'] for k in timed)
    if args.title:
        print(f'== {args.title}')
    shown = kernels if args.all else timed
    for i, k in enumerate(shown):
        others = [o for o in shown if o is not k and o['queue'] != k['queue'] and o['start'] < k['end'] and k['start'] < o['end']]
        if args.brief and k['end'] - k['start'] < 20000:
            continue
        print(f'{k["phase"]:<11} group {k["group"]:>2} queue {k["queue"]:>3} grid {k["grid"]:>8}  {(k["start"] - t0) / 1e6:>9.3f} -> '
              f'{(k["end"] - t0) / 1e6:>9.3f} ms  ({(k["end"] - k["start"]) / 1e6:>7.3f})  {short(k["name"])[:70]}'
              + ('   overlaps ' + ', '.join(sorted({f'{o["phase"]} {o["group"]}' for o in others})) if others else ''))
    spans = {p: [(k['start'], k['end']) for k in timed if k['phase'] == p] for p, _ in PHASES}
    forward, forward_mask = covered(spans['forward'])
    backtrace_alone = outside(spans['backtrace'], forward_mask)
    _, fb_mask = covered(spans['forward'] + spans['backtrace'])
    preparation_alone = outside(spans['preparation'], fb_mask)
    busy, _ = covered([s for p in spans.values() for s in p])
    region = t1 - t0
    per_kernel = {p: sum(b - a for a, b in spans[p]) / 1e6 for p in spans}
    print(f'timed region ({args.groups} groups): {region / 1e6:.3f} ms = forward {forward / 1e6:.3f} + backtrace outside a forward launch '
          f'{backtrace_alone / 1e6:.3f} + preparation outside both {preparation_alone / 1e6:.3f} + idle {(region - busy) / 1e6:.3f}')
    print(f'kernel time summed: forward {per_kernel["forward"]:.3f} ms ({len(spans["forward"])} launches), backtrace '
          f'{per_kernel["backtrace"]:.3f}, preparation {per_kernel["preparation"]:.3f}; forward launches: '
          + ' '.join(f'{(b - a) / 1e6:.3f}' for a, b in spans['forward']))


if __name__ == '__main__':
    main()
