"""The plan a render executes is the plan mtsgpu_plan_host reports (csrc/render_plan.cpp):
after each small render, plan_host for this device's CU count under the same environment
must name the engine and the kernel that ran (debug counter 15) and the launches the sample
count was split into (debug counter 8)."""
import pytest

from mitsuba_amd import scenes
from mitsuba_amd.integrator import plan_host

pytestmark = pytest.mark.gpu

BUDGET = 1 << 20      # the smallest MTSGPU_CONTRIB_BYTES the library takes


def _agree(gpu_ctx, plan, launches=None):
    c = gpu_ctx.debug_counters()
    assert plan['variant_word'] == c[15], (hex(plan['variant_word']), hex(c[15]))
    assert plan['engine'] == ('wavefront' if c[15] & (1 << 16) else 'fields' if c[15] & (1 << 17) else 'megakernel')
    assert plan['launches'] == c[8] == len(plan['launch'])
    if launches is not None:
        assert c[8] == launches


@pytest.mark.parametrize('samples', [False, True], ids=['plain', 'records'])
def test_chunked_cornell_box(gpu_ctx, monkeypatch, samples):
    monkeypatch.setenv('MTSGPU_CONTRIB_BYTES', str(BUDGET))
    sc, it = scenes.build('C1', width=160, height=112, spp=7, rfilter='box')
    gpu_ctx.upload(sc)
    _, _, st = gpu_ctx.render(it, samples=samples)
    assert st['samples'] == 160 * 112 * 7
    plan = plan_host(sc, it, samples=samples, cus=gpu_ctx.scene_info()['cus'])
    _agree(gpu_ctx, plan, launches=3)
    assert plan['variant']['instr'] == samples and gpu_ctx.kernel_variant() == plan['variant']


@pytest.mark.parametrize('engine', [None, 'wavefront'], ids=['megakernel', 'wavefront'])
def test_c3_without_scene_lds(gpu_ctx, monkeypatch, engine):
    monkeypatch.setenv('MTSGPU_NO_SCENE_LDS', '1')
    sc, it = scenes.build('C3', width=40, height=24, spp=8)
    gpu_ctx.upload(sc)
    _, _, st = gpu_ctx.render(it, engine=engine)
    assert st['samples'] == 40 * 24 * 8
    plan = plan_host(sc, it, engine=engine, cus=gpu_ctx.scene_info()['cus'])
    _agree(gpu_ctx, plan, launches=1)
    assert not plan['scene_lds']
    if engine is None:
        assert gpu_ctx.kernel_variant() == plan['variant'] and not plan['variant']['scene_lds']


def test_chunked_field_pass(gpu_ctx, monkeypatch):
    monkeypatch.setenv('MTSGPU_CONTRIB_BYTES', str(BUDGET))
    sc, it = scenes.build('C1', width=96, height=80, spp=5, rfilter='box')
    fields = ['position', 'shNormal', 'primIndex']
    gpu_ctx.upload(sc)
    _, _, st = gpu_ctx.render_fields(it, fields)
    assert st['samples'] == 96 * 80 * 5
    _agree(gpu_ctx, plan_host(sc, it, fields=fields, cus=gpu_ctx.scene_info()['cus']), launches=3)
