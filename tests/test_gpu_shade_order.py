"""k_shade in material order, the queue in the tracer's order ("Sorted shading, queue order kept"): with the
material sort on, k_shade reads each window through the permutation k_sort_queue wrote and the survivors go back to the
next queue in the queue's order.  Which queue position holds a path changes no result, so the sort on and off must give the
same f16 words, on every path that sorts: Standard with the inline light pdf (k_compact_queue appends), Standard with the
light-pdf stage (k_light_pdf appends) and MIS (k_shadow appends).  Each setting runs in a fresh process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORD_FRACTION_TOL = 1e-3   # against the oracle, as tests/test_gpu_parity.py

# multi-family scenes as multi-frame wavefronts (three chained calls = one wavefront by default)
CASES = [dict(key="features1:std", scene="features1", cam=1, type=0, w=96, h=64, frames=3, spp=2, bounces=6),
         dict(key="materials2:std", scene="materials2", cam=1, type=0, w=96, h=64, frames=3, spp=2, bounces=6),
         dict(key="bistro_small:std", scene="bistro_class_small", type=0, w=96, h=64, frames=3, spp=2, bounces=6),
         dict(key="bistro_small:mis", scene="bistro_class_small", type=1, w=96, h=64, frames=3, spp=2, bounces=6),
         dict(key="features1:mis", scene="features1", cam=1, type=1, w=96, h=64, frames=3, spp=2, bounces=6)]


def render(tmp_path, tag, cases, **env_over):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LUPIN_") or k in ("LUPIN_HIP_LIB",)}
    env.update(env_over)
    out = str(tmp_path / f"{tag}.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_shade_order_worker.py"), out, json.dumps(cases)], env=env,
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return np.load(out)


@pytest.fixture(scope="module")
def oracle_images(built):
    imgs = {}
    for c in CASES:
        scene, cams = util.load_scene(c["scene"], None)
        imgs[c["key"]] = util.oracle_accumulate(scene, cams[c.get("cam", 0)], c["w"], c["h"], c["frames"], c["spp"], max_bounces=c["bounces"], ptype=c["type"])
    return imgs


@pytest.mark.gpu
@pytest.mark.parametrize("light_stage", ["0", "1"])
def test_sorted_shading_renders_the_unsorted_images(tmp_path, oracle_images, light_stage):
    on = render(tmp_path, "on", CASES, LUPIN_SORT_SHADE="1", LUPIN_LIGHT_STAGE=light_stage)
    off = render(tmp_path, "off", CASES, LUPIN_SORT_SHADE="0", LUPIN_LIGHT_STAGE=light_stage)
    for c in CASES:
        k = c["key"]
        assert int(on[k + ":frames_per_wavefront"]) == c["frames"], k
        assert util.f16_words_differ(on[k], off[k]) == 0, f"{k}: sort on and off differ"
        nbad = util.f16_words_differ(on[k], oracle_images[k])
        assert nbad <= WORD_FRACTION_TOL * on[k].size, f"{k}: {nbad} f16 words differ from the oracle"


@pytest.mark.gpu
def test_sorted_shading_4k_frame_is_word_for_word_the_unsorted_one(tmp_path, built):
    """The benchmarked frame: bistro-class at 3840 x 2160, 16 bounces, eight chained calls of 8 spp (one wavefront), read once."""
    case = [dict(key="bistro:4k", scene="bistro_class", type=0, w=3840, h=2160, frames=8, spp=8, bounces=16)]
    on = render(tmp_path, "on", case, LUPIN_SORT_SHADE="1")
    off = render(tmp_path, "off", case, LUPIN_SORT_SHADE="0")
    assert int(on["bistro:4k:frames_per_wavefront"]) == 8
    assert np.any(on["bistro:4k"][..., :3] != 0)
    assert util.f16_words_differ(on["bistro:4k"], off["bistro:4k"]) == 0
