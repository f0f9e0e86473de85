#!/usr/bin/env python3
"""Static size of one kernel in hipcc's device assembly (--cuda-device-only -S): code
bytes, VGPRs, SGPRs, spilled SGPRs, scratch, the compiler's occupancy, the static count
of VALU instructions and of v_writelane / v_readlane (the traffic of spilled SGPRs).
The spilled-SGPR count is read from file.txt, the same compile's -Rpass-analysis=
kernel-resource-usage output, where it lies beside file.s.
usage: static_table.py MANGLED_SUBSTRING name=file.s ...   (one row per file)"""
import re
import sys


def sgpr_spill(path, name):
    """the kernel's 'SGPRs Spill' remark in the compile's -Rpass-analysis output, kept beside the
    assembly as <stem>.txt; '?' without that file"""
    try:
        lines = open(path[:-2] + '.txt', errors='replace').read().split('Function Name: ' + name + ' ')
    except OSError:
        return '?'
    m = re.search(r'SGPRs Spill: (\d+)', lines[1]) if len(lines) > 1 else None
    return m.group(1) if m else '?'


def kernel_stats(path, want):
    """the numbers of the first function whose mangled name contains `want`"""
    name, valu, lanes, out = None, 0, 0, None
    for line in open(path, errors='replace'):
        s = line.strip()
        m = re.match(r'(\w+):\s*(;.*)?$', s)
        if m and not line.startswith((' ', '\t', '.')) and name is None and want in m.group(1) and m.group(1).startswith('_Z'):
            name, valu, lanes, out = m.group(1), 0, 0, {}
            continue
        if name is None:
            continue
        if s.startswith('v_'):
            valu += 1
            if s.startswith(('v_writelane', 'v_readlane')):
                lanes += 1
        for key, pat in (('code', r'; codeLenInByte = (\d+)'), ('vgpr', r'; NumVgprs: (\d+)'), ('sgpr', r'; TotalNumSgprs: (\d+)'),
                         ('scratch', r'; ScratchSize: (\d+)'),
                         ('occ', r'; Occupancy: (\d+)')):
            m = re.match(pat, s)
            if m and key not in out:
                out[key] = int(m.group(1))
        if 'occ' in out and 'code' in out:
            out.update(valu=valu, lanes=lanes, name=name, sspill=sgpr_spill(path, name))
            return out
    raise SystemExit('%s: no kernel matching %s' % (path, want))


def main(argv):
    want = argv[0]
    print('%-14s %8s %5s %5s %7s %8s %4s %7s %6s' % ('build', 'code B', 'VGPR', 'SGPR', 'sspill', 'scratch', 'occ', 'VALU', 'lanes'))
    for a in argv[1:]:
        label, path = a.split('=', 1)
        r = kernel_stats(path, want)
        print('%-14s %8d %5d %5d %7s %8d %4d %7d %6d' % (label, r['code'], r['vgpr'], r['sgpr'], r.get('sspill', '?'),
                                                        r['scratch'], r['occ'], r['valu'], r['lanes']))


if __name__ == '__main__':
    main(sys.argv[1:])
