"""bench.py's N-rank launcher (the driver's `python bench.py --gpus N`), rehearsed
on CPU: the parent starts torch.distributed.run with N ranks before touching a
GPU, each rank renders its 8x8 tiles (here with the CPU oracle,
`--device cpu-oracle`; on the GPUs the HIP path with the same tile parameters)
and the films are reduced onto rank 0 (gloo here, RCCL on the GPUs).  The
reduced film must equal the single-process frame bit for bit, at 2, 4 and 8
ranks."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, gpus, name):
    out = str(tmp_path / name)
    env = dict(os.environ, OMP_NUM_THREADS='2')
    env.pop('WORLD_SIZE', None)
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', str(gpus), '--device', 'cpu-oracle',
                        '--config', 'C1', '--size', '40x36x4', '--steps', '2', '--warmup', '1', '--save-film', out],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), np.load(out)


def test_multi_rank_launch_equals_single_process(tmp_path):
    r1, f1 = _bench(tmp_path, 1, 'f1.npy')
    assert r1['n_gpus'] == 1
    for n in (2, 4, 8):
        rn, fn = _bench(tmp_path, n, 'f%d.npy' % n)
        assert rn['n_gpus'] == n and rn['config']['world_size_reported'] == n
        assert rn['config']['samples_per_frame'] == r1['config']['samples_per_frame'] == 40 * 36 * 4
        assert np.array_equal(f1.view(np.uint32), fn.view(np.uint32)), n


def _plain(tmp_path, name, *extra):
    """A one-rank run at 40x36x4 with --dump-outputs (and --save-film), as the driver starts it."""
    d = tmp_path / name
    env = dict(os.environ, OMP_NUM_THREADS='2')
    env.pop('WORLD_SIZE', None)
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--device', 'cpu-oracle',
                        '--config', 'C1', '--size', '40x36x4', '--steps', '3', '--warmup', '0',
                        '--dump-outputs', str(d), '--save-film', str(tmp_path / (name + '.npy'))] + list(extra),
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), d


def test_dump_outputs_is_the_last_steps_film_and_repeats(tmp_path):
    """--dump-outputs DIR writes the reduced film of the last timed step as DIR/film.npy
    (float32, within the 64 MB budget), the same array --save-film writes, and a second
    run with the same arguments writes the same bits; a plain run carries the headline
    fields and none of what --full adds."""
    ra, da = _plain(tmp_path, 'a')
    rb, db = _plain(tmp_path, 'b')
    assert sorted(os.listdir(da)) == ['film.npy']
    fa, fb = np.load(da / 'film.npy'), np.load(db / 'film.npy')
    assert fa.dtype == np.float32 and fa.shape == (36 + 2, 40 + 2, 5)      # the box filter's border of 1
    assert fa.nbytes <= 64e6 and fa[1:-1, 1:-1].any()
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    assert np.array_equal(fa.view(np.uint32), np.load(tmp_path / 'a.npy').view(np.uint32))
    assert ra['steps'] == 3 and ra['warmup'] == 0 and ra['ms_per_step'] > 0
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in ra, k
    assert ra['full'] is False and 'secondary' not in ra and ra['roofline'] is None and ra['cpu_baseline'] is None


def test_steps_must_be_positive(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--device', 'cpu-oracle',
                        '--steps', '0'], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and '--steps' in p.stderr


def test_world_size_mismatch_fails(tmp_path):
    env = dict(os.environ, WORLD_SIZE='2', RANK='0', LOCAL_RANK='0')
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '4', '--device', 'cpu-oracle'],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and 'WORLD_SIZE' in p.stderr
