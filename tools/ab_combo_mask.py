#!/usr/bin/env python3
"""C5 with its ground (both checker colours) wrapped in mask(opacity = 1) next to plain C5.

mask(opacity = 1) is the identity (tests/test_gpu_combo.py::test_mask_identity), so the two
renders compute the same film; the wrapped scene runs the MTSG_FEAT_SET_COMBO kernels
(dcombo.h), plain C5 its BSDF-set megakernel.  The renders alternate in one process, each
timed by the library's own kernel time; the line printed per engine is the median of the
repeats in Msamples/s.  No gate: nobody has a target for a combinator scene.

usage: ab_combo_mask.py [--width W --height H --spp N --repeats R]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pkgimport import mitsuba_amd  # noqa: E402

mitsuba_amd()
from mitsuba_amd import scenes  # noqa: E402
from mitsuba_amd.integrator import Context, kernel_variant_of  # noqa: E402
from mitsuba_amd.scene import BSDF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--height', type=int, default=720)
    ap.add_argument('--spp', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    plain, it = scenes.build('C5', width=a.width, height=a.height, spp=a.spp)
    it.rfilter = 'box'
    import copy
    wrapped = copy.copy(plain)
    wrapped.bsdfs = [plain.bsdfs[0]] + [BSDF('mask', opacity=1.0, nested=[b]) for b in plain.bsdfs[1:]]
    ctx = Context()
    for engine in (None, 'wavefront'):
        rate = {'plain': [], 'mask': []}
        films = {}
        for r in range(a.repeats + 1):      # the first round warms up
            for name, sc in (('plain', plain), ('mask', wrapped)):
                ctx.upload(sc)
                film, _, st = ctx.render(it, engine=engine)
                word = ctx.debug_counters()[15]
                if r:
                    rate[name].append(st['samples'] / st['kernel_ms'] / 1e3)
                films[name] = (film, word)
        same = np.array_equal(films['plain'][0].view(np.uint32), films['mask'][0].view(np.uint32))
        for name in ('plain', 'mask'):
            v = kernel_variant_of(films[name][1])
            print('%s %-5s %s: median %.1f Msamples/s (min %.1f, max %.1f, n = %d)' % (
                engine or 'megakernel', name, v['name'] if v else hex(films[name][1]), float(np.median(rate[name])),
                min(rate[name]), max(rate[name]), len(rate[name])))
        print('%s films bit-identical: %s' % (engine or 'megakernel', same))


if __name__ == '__main__':
    main()
