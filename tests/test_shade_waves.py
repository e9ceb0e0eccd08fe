"""k_shade at four waves per SIMD ("k_shade at four waves"): the inline Standard / Direct kernels evaluate
everything that reads the surface before the light-pdf march and share one copy of the march between the surface and the
in-medium mixture.  The register budget is checked on the built library; the images stay the oracle's word for word on the
scenes where the reordered statements meet (a medium pushed or popped in the vertex of a march, opacity and normal maps under
the permuted shading order, the LDS-staged instantiation, many emissive instances over chained frames)."""
import os
import re
import subprocess
import sys

import pytest

from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+) code\s+(\d+)\s+void (k_shade<[^>]*>)")


def shade_resources(text):
    """{instantiation: (vgprs, scratch bytes)} of the k_shade lines of a tools/kernel_resources.py listing."""
    return {m.group(6).replace(" ", ""): (int(m.group(1)), int(m.group(3))) for m in map(LINE.search, text.split("\n")) if m}


@pytest.fixture(scope="module")
def built_resources(built):
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_shade"], text=True)
    return shade_resources(out)


@pytest.mark.parametrize("ldsgeo", ["true", "false"])
def test_standard_shade_fits_four_waves(built_resources, ldsgeo):
    vgprs, scratch = built_resources[f"k_shade<0,{ldsgeo},false,false>"]
    print(f"k_shade<0,{ldsgeo},false,false>: {vgprs} VGPRs, {scratch} B scratch")
    assert vgprs <= 128 and scratch == 0


@pytest.mark.parametrize("ldsgeo", ["true", "false"])
def test_direct_shade_did_not_grow(built_resources, ldsgeo):
    with open(os.path.join(ROOT, "profiles", "surface_probe_kernel_resources_after.txt")) as f:
        was = shade_resources(f.read())[f"k_shade<3,{ldsgeo},false,false>"]
    now = built_resources[f"k_shade<3,{ldsgeo},false,false>"]
    print(f"k_shade<3,{ldsgeo},false,false>: {was} -> {now} (VGPRs, scratch bytes)")
    assert now[0] <= was[0] and now[1] <= was[1]


# materials4: volumetric and refractive materials under an area light -- a medium pushed and popped in the vertex of a march;
# features1: opacity, normal map, >= 4 BSDF families (permuted shading order); the Cornell box: geometry staged in LDS
@pytest.mark.gpu
@pytest.mark.parametrize("name,width,height", [("materials4", 96, 64), ("features1", 96, 64), ("cornellbox_builtin", 64, 64)])
@pytest.mark.parametrize("ptype", [0, 3], ids=["standard", "direct"])
def test_shade_equals_oracle(gpu_ctx, name, width, height, ptype):
    scene, cams = util.load_scene(name, gpu_ctx)
    got = util.gpu_accumulate(gpu_ctx, scene, cams[0], width, height, frames=2, spp=4, max_bounces=8, ptype=ptype)
    ref = util.oracle_accumulate(scene, cams[0], width, height, frames=2, spp=4, max_bounces=8, ptype=ptype)
    assert util.f16_words_differ(got, ref) == 0


@pytest.mark.gpu
def test_bistro_class_chained_and_single_frames(gpu_ctx):
    """Many emissive instances, 16 bounces: the default wavefront of chained frames, one frame per wavefront and the oracle."""
    scene, cams = util.load_scene("bistro_class_small", gpu_ctx)
    W, H = 120, 80
    chained = util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=3, spp=2, max_bounces=16)
    gpu_ctx.set_batch_frames(1)
    try:
        single = util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=3, spp=2, max_bounces=16)
    finally:
        gpu_ctx.set_batch_frames(0)
    assert util.f16_words_differ(chained, single) == 0
    ref = util.oracle_accumulate(scene, cams[0], W, H, frames=3, spp=2, max_bounces=16)
    assert util.f16_words_differ(chained, ref) == 0
