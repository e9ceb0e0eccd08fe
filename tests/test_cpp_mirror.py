"""Every entry point of the C++ host mirror (include/lupin.hpp) that no example calls, run by tests/cpp_mirror_probe.cpp and
compared with the Python host (lupinpathtracer_amd.api) on the same inputs, through the same library: the words are equal.
The kernels underneath are held to float64 references through the Python host elsewhere; here the two hosts are held to
each other, so a descriptor filled in another order than include/lupin_hip.h declares, or host arithmetic that rounds
differently, shows.  Without a device: the program compiles, the host-only entry points, every default, and a guard that a
wrapper added to the header has a section."""
import dataclasses
import enum
import inspect
import os
import re
import subprocess
import time

import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import cpp_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lupin.hpp")
SOURCE = os.path.join(ROOT, "tests", "cpp_mirror_probe.cpp")
EXE = os.path.join(ROOT, "tests", "cpp_mirror_probe")
# -ffp-contract=off and no -march=native: the header's host arithmetic is separately rounded f32 operations, as numpy's is
FLAGS = ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]


def compile_probe(header_dir, exe):
    lib_dir = os.path.join(ROOT, "lupinpathtracer_amd")
    subprocess.check_call(["g++", *FLAGS, "-I" + header_dir, SOURCE, "-L" + lib_dir, "-llupin_hip", "-L/opt/rocm/lib", "-lz", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def probe(built):
    return compile_probe(os.path.join(ROOT, "include"), EXE)


def run_probe(exe, tmp, arrays, sections=()):
    inputs, outputs = os.path.join(tmp, "inputs.bin"), os.path.join(tmp, "outputs.bin")
    M.write_blob(inputs, arrays)
    p = subprocess.run([exe, inputs, outputs, *sections], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return M.read_blob(outputs)


def sections_of(exe):
    """{section: the lp:: names it runs}, as the program lists them."""
    lines = subprocess.run([exe, "--list"], capture_output=True, text=True, check=True).stdout.splitlines()
    return {line.split(":")[0]: line.split(":")[1].split() for line in lines}


def words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_same_words(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = int((words(got) != words(want)).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} words differ between the C++ host and the Python host"


# ---- without a device ---------------------------------------------------------------------------------------------

def test_the_blob_round_trips(tmp_path):
    arrays = {"a": np.arange(6, dtype=np.float32).reshape(2, 3), "b.c": np.array([7], np.uint32), "d": np.zeros((0, 4), np.uint8),
              "e": np.arange(5, dtype=np.uint16)}
    path = str(tmp_path / "blob.bin")
    M.write_blob(path, arrays)
    back = M.read_blob(path)
    assert list(back) == list(arrays)
    for k in arrays:
        assert back[k].dtype == arrays[k].dtype and np.array_equal(back[k], arrays[k])


def test_the_inputs_keep_same_typed_fields_apart(built):
    """Inputs() asserts the rule for every descriptor while it builds them; and the rule itself refuses what it must."""
    M.Inputs()
    with pytest.raises(AssertionError):
        M.distinct("BentNormalDesc", samples=4, flags=0, max_slots=4, ray_epsilon=0.002)
    with pytest.raises(AssertionError):
        M.distinct("LupinAdvancedParams", max_radiance=0.002, rng_seed=7, ray_epsilon=0.002)
    M.distinct("mixed", samples=2, ray_epsilon=2.0)


@pytest.fixture(scope="module")
def host_only(probe, tmp_path_factory):
    arrays = M.host_inputs()
    return arrays, run_probe(probe, str(tmp_path_factory.mktemp("host_only")), arrays, ["host_only"])


def test_probe_grid_positions_equal_the_python_hosts(host_only):
    arrays, got = host_only
    want = api.probe_grid_positions(arrays["host_only.grid.origin"], arrays["host_only.grid.spacing"], arrays["host_only.grid.dims"])
    assert want.shape == (24, 3)
    assert_same_words(got["host_only.probe_grid_positions"], want, "probe_grid_positions")
    # the inputs tell the product first from the sum first
    o, s = arrays["host_only.grid.origin"], arrays["host_only.grid.spacing"]
    other = np.array([(o[k] + np.arange(4, dtype=np.float32)) * s[k] for k in range(3)])
    first = np.array([o[k] + np.arange(4, dtype=np.float32) * s[k] for k in range(3)])
    assert (words(other) != words(first)).any()


def sh_terms(coeffs, normals):
    """Per (point, coefficient, channel) the float64 products c_j * A_j * Y_j(n) of sh_irradiance's sum, written out here from
    the formula (Ramamoorthi-Hanrahan: the real harmonics 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2 with their
    normalisations, times the clamped cosine's band factors pi, 2 pi / 3, pi / 4), not taken from either host."""
    n = np.asarray(normals, np.float64)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    pi = np.pi
    basis = np.stack([np.full_like(x, 0.5 * np.sqrt(1.0 / pi)),
                      np.sqrt(3.0 / (4.0 * pi)) * y, np.sqrt(3.0 / (4.0 * pi)) * z, np.sqrt(3.0 / (4.0 * pi)) * x,
                      0.5 * np.sqrt(15.0 / pi) * x * y, 0.5 * np.sqrt(15.0 / pi) * y * z, 0.25 * np.sqrt(5.0 / pi) * (3.0 * z * z - 1.0),
                      0.5 * np.sqrt(15.0 / pi) * x * z, 0.25 * np.sqrt(15.0 / pi) * (x * x - y * y)], axis=1)
    band = np.array([pi, 2.0 * pi / 3.0, 2.0 * pi / 3.0, 2.0 * pi / 3.0, pi / 4.0, pi / 4.0, pi / 4.0, pi / 4.0, pi / 4.0])
    return np.asarray(coeffs, np.float64)[..., :3] * (basis * band)[..., None]


def test_sh_irradiance_against_float64_and_the_python_host(host_only):
    """The header's function is, per channel, nine products and eight additions in f32, each term's factor A_j Y_j(n) built
    from at most five more f32 operations on constants rounded to f32 (a2 * (k3 * ((3 nz) nz - 1)) is the longest: five
    roundings of the operations and two of the constants).  Along the longest chain a term therefore passes 7 roundings of
    its factor, 1 of its product with c_j and 8 of the running sum: k = 16 roundings of relative size 2^-24 each, applied to
    sums whose magnitude is at most sum_j |c_j A_j Y_j|.  (The -1 of the band-2 zonal term can cancel against 3 nz^2; its
    absolute error is bounded by the same roundings of the larger operand, 3 k3 a2 |c| <= 2.4 |c| wide, which the bound
    takes in by adding the uncancelled magnitude |c_6| a2 k3 (3 nz^2 + 1) for that term.)"""
    arrays, got = host_only
    coeffs, normals = arrays["host_only.sh.coeffs"], arrays["host_only.sh.normals"]
    terms = sh_terms(coeffs, normals)
    exact = terms.sum(axis=1)
    magnitude = np.abs(terms)
    a2k3 = (np.pi / 4.0) * 0.25 * np.sqrt(5.0 / np.pi)
    magnitude[:, 6, :] = np.abs(np.asarray(coeffs, np.float64)[:, 6, :3]) * a2k3 * (3.0 * normals[:, 2:3].astype(np.float64) ** 2 + 1.0)
    bound = 16 * 2.0 ** -24 * magnitude.sum(axis=1)
    cpp = got["host_only.sh_irradiance"]
    assert cpp.dtype == np.float32 and cpp.shape == (64, 3)
    err = np.abs(cpp.astype(np.float64) - exact)
    print("sh_irradiance: worst |C++ - float64| / bound =", float((err / bound).max()))
    assert (err <= bound).all()
    py = api.sh_irradiance(coeffs, normals)     # float64 as well, summed in another order
    assert py.dtype == np.float64 and (np.abs(cpp.astype(np.float64) - py) <= bound).all()
    assert (np.abs(exact) > 100 * bound).mean() > 0.9      # the bound is no licence: most sums stand far above it


def test_host_only_counts_and_refusals(host_only):
    arrays, got = host_only
    tiles = arrays["host_only.get_num_tiles"]
    assert np.array_equal(got["host_only.num_tiles"], [api.get_num_tiles(int(t), int(w), int(h)) for t, w, h in tiles])
    # validate_scene: the valid scene passes, each broken one is refused with LUPIN_ERR_INVALID_ARGUMENT
    assert got["host_only.validate_scene"].tolist() == [0, 1, 1, 1, 1, 1]
    # a segment of length exactly 2 * ray_epsilon is refused by segment_records, visible and transmittance, without a device
    assert got["host_only.short_refused"].tolist() == [1, 1, 1]
    with pytest.raises(ValueError):
        api.segment_records(arrays["host_only.short.p"], arrays["host_only.short.q"], arrays["host_only.segments.ray_epsilon"])


def test_segment_records_equal_the_python_hosts(host_only):
    """The arithmetic visible and transmittance share (d = q - p, its length, the division, tmax = len - ray_epsilon)."""
    arrays, got = host_only
    want = api.segment_records(arrays["host_only.segments.p"], arrays["host_only.segments.q"], arrays["host_only.segments.ray_epsilon"])
    assert_same_words(got["host_only.segment_records"], want, "segment_records")


# C++ defaults that differ from the Python host's on purpose, or that the Python host has no default for: the C++ value and why
DELIBERATE = {
    "ProbeGridDesc.normal_bias": (0.0, "lupin.hpp: 'world units; the Python mirror's default is 1e-4 of the scene's extent' (None there)"),
    "BakedViewDesc.grid.normal_bias": (0.0, "ProbeGridDesc's, as above"),
    "BakedViewDesc.grid.flags": (6, "ProbeGridDesc's: 'and without maps LUPIN_PROBE_GRID_VISIBILITY (clear it with maps)'; render_baked's visibility is False"),
    "BakedViewDesc.resolution": (16, "lupin.hpp: 'of the maps; with depth only'; the Python host reads it off the maps' shape"),
    "BakedViewDesc.max_distance": (1.0, "lupin.hpp: 'the maps' bake's; with depth only'; None in the Python host"),
    "BakedViewDesc.flags": (0, "device pointers: the Python host decides by the arguments' types"),
    "ProbeGridDesc.origin": ([0.0, 0.0, 0.0], "a required argument of the Python host"),
    "ProbeGridDesc.spacing": ([1.0, 1.0, 1.0], "a required argument of the Python host"),
    "ProbeGridDesc.dims": ([1, 1, 1], "a required argument of the Python host"),
    "BakedViewDesc.grid.origin": ([0.0, 0.0, 0.0], "a required argument of the Python host"),
    "BakedViewDesc.grid.spacing": ([1.0, 1.0, 1.0], "a required argument of the Python host"),
    "BakedViewDesc.grid.dims": ([1, 1, 1], "a required argument of the Python host"),
    "LightmapAoDesc.width": (0, "a required argument of the Python host"),
    "LightmapAoDesc.height": (0, "a required argument of the Python host"),
    "LightmapAoDesc.surface_offset": (0.0, "lupin.hpp: 'the caller chooses (> 0)'; None in the Python host: 1e-4 of the scene's extent"),
    "LightmapDenoiseDesc.width": (0, "the Python host reads it off the atlas' shape"),
    "LightmapDenoiseDesc.height": (0, "the Python host reads it off the atlas' shape"),
    "LightmapDenoiseDesc.flags": (0, "device pointers: the Python host decides by the arguments' types"),
    "OcclusionDesc.flags": (0, "device pointers: the Python host decides by the arguments' types"),
    "BentNormalDesc.samples": (64, "a required argument of the Python host; ambient_occlusion's default there"),
}


def plain(v):
    if v is None:
        return 0            # an absent optional: the probe writes whether it has a value
    if isinstance(v, (bool, enum.Enum)):
        return int(v)
    return v


def dataclass_defaults(cls, prefix):
    out = {}
    for f in dataclasses.fields(cls):
        if f.default is not dataclasses.MISSING:
            v = f.default
        elif f.default_factory is not dataclasses.MISSING:
            v = f.default_factory()
        else:
            continue        # a required field
        if dataclasses.is_dataclass(v):
            out.update(dataclass_defaults(type(v), f"{prefix}.{f.name}"))
        else:
            out[f"{prefix}.{f.name}"] = plain(v)
    return out


def argument_defaults(fn, prefix):
    return {f"{prefix}.{name}": plain(p.default) for name, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def python_defaults():
    out = {}
    for name in ("BakedPathtraceParams", "CameraParams", "AdvancedParams", "TileParams", "PathtraceDesc", "DebugVizDesc", "TonemapDesc", "Viewport", "DenoiseDesc",
                 "AdaptiveParams", "ReprojectDesc", "RayQueryDesc", "LightmapChart", "LightmapDesc", "ProbeDesc", "ProbeDepthDesc"):
        out.update(dataclass_defaults(getattr(api, name), name))
    for name, fn in (("LightmapAdaptiveDesc", api.bake_lightmap_adaptive), ("LightmapAoDesc", api.bake_lightmap_ao), ("LightmapDenoiseDesc", api.denoise_lightmap),
                     ("OcclusionDesc", api.occlusion_rays), ("BentNormalDesc", api.bent_normal_rays), ("ProbeGridDesc", api.sample_probe_grid),
                     ("BakedViewDesc", api.render_baked), ("BakedViewDesc.grid", api.render_baked)):
        out.update(argument_defaults(fn, name))
    # what the Python host spells as booleans, and the view's camera, which it takes as the dataclasses the frames take
    g = inspect.signature(api.sample_probe_grid).parameters
    out["ProbeGridDesc.flags"] = api.PROBE_GRID_VISIBILITY * g["visibility"].default + api.PROBE_GRID_BACKFACE * g["backface"].default
    v = inspect.signature(api.render_baked).parameters
    out["BakedViewDesc.grid.flags"] = api.PROBE_GRID_VISIBILITY * v["visibility"].default + api.PROBE_GRID_BACKFACE * v["backface"].default
    a = inspect.signature(api.bake_lightmap_ao).parameters
    out["LightmapAoDesc.flags"] = api.LIGHTMAP_SMOOTH_NORMALS * a["smooth_normals"].default + api.LIGHTMAP_AO_OPACITY * a["opacity"].default
    out["BentNormalDesc.flags"] = api.BENT_NORMAL_OPACITY * inspect.signature(api.bent_normal_rays).parameters["opacity"].default
    out.update(dataclass_defaults(api.CameraParams, "BakedViewDesc.camera_params"))
    out["BakedViewDesc.camera_transform"] = api.identity_mat3x4()
    for k in ("ProbeGridDesc.normal_bias", "BakedViewDesc.grid.normal_bias", "BakedViewDesc.max_distance", "LightmapAoDesc.surface_offset"):
        assert out.pop(k) == 0     # None there: computed per call, no value to compare
    return out


def test_defaults_equal_the_python_hosts(probe, tmp_path):
    got = run_probe(probe, str(tmp_path), {}, ["defaults"])
    got.pop("done.defaults")
    assert len(got) > 100
    py = python_defaults()
    unlisted, needless = [], []
    for name, value in got.items():
        value = value.reshape(-1) if value.size > 1 else value.reshape(())
        if name in py:
            same = np.array_equal(value, np.asarray(py[name], value.dtype).reshape(value.shape))
        else:
            same = False
        if name in DELIBERATE:
            assert np.array_equal(value, np.asarray(DELIBERATE[name][0], value.dtype)), f"{name}: the table pins {DELIBERATE[name][0]}, the header says {value}"
            if same:
                needless.append(name)
        elif not same:
            unlisted.append(f"{name}: C++ {value.tolist()}, Python {py.get(name, 'has none')}")
    assert not unlisted, "defaults that differ from the Python host's and are not listed as deliberate:\n" + "\n".join(unlisted)
    assert not needless, f"listed as deliberate, but equal: {needless}"
    assert not set(DELIBERATE) - set(got), f"listed as deliberate, but not a default of the header: {set(DELIBERATE) - set(got)}"


# free functions of namespace lp that the examples run (tests/test_cpp_host.py compares their images with the Python host's)
COVERED_BY_EXAMPLES = {"check", "mat3x4_identity", "default_mesh_info", "default_instance", "default_material", "build_pathtrace_resources",
                       "build_accel_structures_and_upload", "pathtrace_scene", "tonemap_and_fit_aspect"}
# needs more than one device to mean anything; tests/_gather_worker.py covers the C ABI underneath
OUT_OF_SCOPE = {"gather_framebuffer_all"}


def test_every_wrapper_of_the_header_has_a_section(probe):
    text = open(HEADER).read()
    lp = text[text.index("namespace lp {"):text.index("}  // namespace lp")]
    # namespace detail holds what the wrappers share (the descriptor conversions): it runs when they run
    api_only = re.sub(r"^namespace detail \{.*?^\}  // namespace detail$", "", lp, flags=re.M | re.S)
    assert "inline void fill_desc(" not in api_only and "inline void fill_desc(" in lp
    names = set(re.findall(r"^inline [^\n(]*?(\w+)\(", api_only, re.M))
    assert {"bent_normal_rays", "render_lightmapped_directional", "visible", "sh_irradiance", "pathtrace_scene"} <= names and len(names) > 45
    listed = sections_of(probe)
    covered = set().union(*listed.values())
    assert "update_instances" in covered           # Scene::update_instances is a member: the regex does not see it
    missing = names - covered - COVERED_BY_EXAMPLES - OUT_OF_SCOPE
    assert not missing, f"include/lupin.hpp has wrappers that tests/cpp_mirror_probe.cpp does not run: {sorted(missing)}"
    source = open(SOURCE).read()
    for section, covers in listed.items():      # what a section says it runs, it calls
        for name in covers:
            call = r"\.update_instances\(" if name == "update_instances" else r"\blp::" + name + r"\("
            assert re.search(call, source), f"section {section} lists {name}, and the program never calls it"
    stale = (covered - {"update_instances"}) - names
    assert not stale, f"the probe lists names the header does not have: {sorted(stale)}"
    examples = "".join(open(os.path.join(ROOT, "examples", f)).read() for f in ("example1.cpp", "render_scene.cpp")) + open(
        os.path.join(ROOT, "include", "lupin_loader.hpp")).read() + text
    for name in COVERED_BY_EXAMPLES:
        assert len(re.findall(r"\b" + name + r"\(", examples)) > 1, f"{name} is listed as run by the examples, and nothing calls it"


# ---- on the device ------------------------------------------------------------------------------------------------

DEVICE_SECTIONS = ["baked_view_desc_c", "pathtrace_scene_tiles", "pathtrace_scene_falsecolor", "pathtrace_scene_debug", "denoise", "pathtrace_scene_adaptive",
                   "adaptive_reproject", "pathtrace_rays", "pathtrace_rays_moments", "bake_probes", "occlusion_rays", "visible", "ambient_occlusion",
                   "bent_normal_rays", "distance_points", "bake_distance_grid", "sample_probe_grid", "bake_probe_depth", "sample_probe_grid_depth", "render_baked",
                   "update_instances", "transmittance_rays", "transmittance", "bake_lightmap", "bake_lightmap_directional", "bake_lightmap_adaptive", "bake_lightmap_ao",
                   "denoise_lightmap", "render_lightmapped", "render_lightmapped_directional"]


def test_the_device_sections_are_the_programs(probe):
    assert set(DEVICE_SECTIONS) | {"host_only", "defaults"} == set(sections_of(probe))


@pytest.fixture(scope="module")
def both_hosts(gpu_ctx, probe, tmp_path_factory):
    """(the Python host, the probe's outputs): the program runs once, for every section."""
    inputs = M.Inputs()
    host = M.PythonHost(gpu_ctx, inputs)
    inputs.set_adaptive_threshold(host.pick_adaptive_threshold())
    t = time.perf_counter()
    got = run_probe(probe, str(tmp_path_factory.mktemp("cpp_mirror")), inputs.blob)
    print(f"cpp_mirror_probe: {time.perf_counter() - t:.2f} s for {len(DEVICE_SECTIONS) + 2} sections")
    return host, got


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEVICE_SECTIONS)
def test_section_equals_the_python_host_word_for_word(both_hosts, name):
    host, got = both_hosts
    assert got[f"done.{name}"] == 1
    want = host.section(name)
    mine = {k: v for k, v in got.items() if k.startswith(name + ".")}
    assert set(mine) == set(want), f"{name}: the probe wrote {sorted(mine)}, the Python host gives {sorted(want)}"
    for k in sorted(want):
        assert_same_words(mine[k], want[k], k)
    SECTION_CHECKS.get(name, lambda host, out: None)(host, mine)


def check_adaptive(host, out):
    """Some 8 x 8 blocks stopped before the third call and some did not."""
    a = host.P["pathtrace_scene_adaptive"]
    pixels = a["width"] * a["height"]
    frames = out["pathtrace_scene_adaptive.frames"]
    assert frames.shape == (a["height"], a["width"]) and a["calls"] == 3
    assert 2 * pixels < int(frames.sum()) < 3 * pixels and frames.min() == 2 and frames.max() == 3
    assert int(out["pathtrace_scene_adaptive.stats"][1]) == int(frames.sum())


def check_transmittance(host, out):
    t = out["transmittance.t"]
    assert ((t > 0) & (t < 1)).sum() >= 4, "no segment crosses a half-transparent surface"


def check_tiles(host, out):
    """tile_size counts 4 x 4 pixel workgroups.  With tile_size 16 the 40 x 24 frame is a single tile of 64 x 64 pixels, which
    rank 0 owns: rank 1 of 2 writes nothing, on either host.  With tile_size 4 (16 pixels) the frame is 3 x 2 tiles, the last
    column and the last row cut off by the frame; rank 1 owns tiles 1, 3 and 5 and leaves the others as they were."""
    p = host.P["pathtrace_scene_tiles"]
    assert api.get_num_tiles(p["tile_size"], p["width"], p["height"]) == 1 and not out["pathtrace_scene_tiles.image.tile_size"].any()
    assert api.get_num_tiles(p["small_tile_size"], p["width"], p["height"]) == 6
    lit = (out["pathtrace_scene_tiles.image.small_tile_size"] != 0).any(axis=-1)
    assert int(lit.sum()) == 16 * 16 + 16 * 8 + 8 * 8        # a whole tile, one cut by the last row, one cut by both edges


def check_lightmap(host, out):
    covered = int(out["bake_lightmap.covered"][0])
    assert M.ATLAS[0] * M.ATLAS[1] // 8 < covered < M.ATLAS[0] * M.ATLAS[1]
    owners = out["bake_lightmap.rgba"][..., 3] == 1.0
    assert owners[:M.ATLAS[1] // 2, :M.ATLAS[0] // 2].any() and owners[M.ATLAS[1] // 2 + 1:, M.ATLAS[0] // 2 + 1:].any()     # both charts own texels


def check_distance(host, out):
    found = out["distance_points.found"]
    assert 0 < found.sum() < len(found)         # some of the bounded searches find nothing


SECTION_CHECKS = {"pathtrace_scene_adaptive": check_adaptive, "transmittance": check_transmittance, "pathtrace_scene_tiles": check_tiles,
                  "bake_lightmap": check_lightmap, "distance_points": check_distance}
