#!/usr/bin/env python3
"""Tabulate the compiler's kernel-resource-usage remarks of a build.

The Makefile keeps every kernel object's -Rpass-analysis=kernel-resource-usage
output in mitsuba0.6_amd/_build/*.resource.txt.  This prints one line per kernel
instantiation, sorted by name:

    <object> <mangled kernel> sgpr=.. vgpr=.. agpr=.. scratch=.. occ=.. sspill=.. vspill=.. lds=..

usage: resource_all.py [BUILD_DIR] [--skip SUBSTRING ...]

Two builds' tables compare with diff(1): a change that must not touch the
existing kernels leaves every line it shares with the parent's table identical.
--skip drops the kernels whose mangled name contains SUBSTRING (a new feature
set's instantiations, say).
"""
import glob
import os
import re
import sys

KEYS = (('TotalSGPRs', 'sgpr'), ('VGPRs', 'vgpr'), ('AGPRs', 'agpr'), ('ScratchSize [bytes/lane]', 'scratch'),
        ('Occupancy [waves/SIMD]', 'occ'), ('SGPRs Spill', 'sspill'), ('VGPRs Spill', 'vspill'),
        ('LDS Size [bytes/block]', 'lds'))
REMARK = re.compile(r'remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]')


def table(build_dir, skip=()):
    rows = []
    for path in sorted(glob.glob(os.path.join(build_dir, '*.resource.txt'))):
        obj = os.path.basename(path)[:-len('.resource.txt')]
        cur = None
        for line in open(path, errors='replace'):
            m = REMARK.search(line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2)
            if key == 'Function Name':
                cur = {'name': val}
                rows.append((obj, cur))
            elif cur is not None:
                cur[key] = val
    out = []
    for obj, r in rows:
        if any(s in r['name'] for s in skip):
            continue
        out.append('%s %s %s' % (obj, r['name'], ' '.join('%s=%s' % (short, r.get(k, '?')) for k, short in KEYS)))
    return sorted(out)


def main(argv):
    skip, args = [], []
    it = iter(argv)
    for a in it:
        if a == '--skip':
            skip.append(next(it))
        else:
            args.append(a)
    here = os.path.dirname(os.path.abspath(__file__))
    build = args[0] if args else os.path.join(here, '..', 'mitsuba0.6_amd', '_build')
    print('\n'.join(table(build, skip)))


if __name__ == '__main__':
    main(sys.argv[1:])
