#!/usr/bin/env python3
"""Cuts the fixtures the suite needs from a Mitsuba 0.6 source tree, so that no
test reads anything outside the repository:

  reference_names.json      the class registry (the abstract and the concrete names
                            of every MTS_IMPLEMENT_CLASS[_S]) and the plugin names
                            (src/**/<name>.cpp): names only, for test_shim_literals.py
  bunny.ply.xz              data/tests/bunny.ply (test_reference_bunny.py)
  microfacet/<d>.dat.xz     data/microfacet/{beckmann,ggx,phong}.dat, the rough-
                            transmittance tables roughplastic reads
                            (test_roughplastic_host.py, test_oracle_bsdf.py)

Data files are stored whole, xz-compressed (each under 1 MiB); tests/conftest.py
unpacks them into a temporary directory.

    python tests/golden/make_reference_fixtures.py <mitsuba source tree>
"""
import json
import lzma
import os
import re
import sys
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = ['data/tests/bunny.ply', 'data/microfacet/beckmann.dat', 'data/microfacet/ggx.dat', 'data/microfacet/phong.dat']


def registry(ref):
    reg = {}
    pat = re.compile(r'MTS_IMPLEMENT_CLASS(?:_S)?\(\s*(\w+)\s*,\s*(true|false)\s*,')
    for root in ('src', 'include'):
        for dp, _, fns in os.walk(os.path.join(ref, root)):
            for fn in fns:
                if fn.endswith(('.cpp', '.h', '.inl')):
                    with open(os.path.join(dp, fn), errors='replace') as f:
                        for m in pat.finditer(f.read()):
                            reg[m.group(1)] = reg.get(m.group(1), True) and m.group(2) == 'true'
    return reg


def plugins(ref):
    return sorted({fn[:-4] for _, _, fns in os.walk(os.path.join(ref, 'src')) for fn in fns if fn.endswith('.cpp')})


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    reg = registry(ref)
    lists = {'abstract': sorted(n for n, a in reg.items() if a), 'concrete': sorted(n for n, a in reg.items() if not a),
             'plugins': plugins(ref)}
    with open(os.path.join(HERE, 'reference_names.json'), 'w') as f:   # one wrapped list per key
        f.write('{\n' + ',\n'.join('"%s": [\n%s\n]' % (k, textwrap.fill(json.dumps(v)[1:-1], 110))
                                   for k, v in lists.items()) + '\n}\n')
    for rel in DATA:
        sub = 'microfacet' if '/microfacet/' in rel else ''
        os.makedirs(os.path.join(HERE, sub), exist_ok=True)
        out = os.path.join(HERE, sub, os.path.basename(rel) + '.xz')
        raw = open(os.path.join(ref, rel), 'rb').read()
        packed = lzma.compress(raw, preset=9 | lzma.PRESET_EXTREME)
        assert len(packed) < (1 << 20), (rel, len(packed))
        with open(out, 'wb') as f:
            f.write(packed)
        print('%s: %d -> %d bytes' % (rel, len(raw), len(packed)))


if __name__ == '__main__':
    main()
