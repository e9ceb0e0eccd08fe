// stitch_mirror_probe.cpp -- runs the C++ host mirror of lightmap seam stitching (include/lupin_stitch.hpp) on inputs read
// from a blob and writes every output to a blob; tests/test_stitch_mirror.py makes the same calls through the Python host and
// compares the words.  The blob format is tests/cpp_mirror_probe.cpp's.
//
//   stitch_mirror_probe <inputs.bin> <outputs.bin> [section ...]     no section names: every section
//   stitch_mirror_probe --list                                       one line per section: its name, then the lp:: names it runs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "lupin_loader.hpp"
#include "lupin_stitch.hpp"

namespace {

enum Dtype : uint32_t { F32 = 0, U32 = 1 };
struct Array { uint32_t dtype = F32; std::vector<uint64_t> dims; std::vector<uint8_t> bytes; };
std::vector<std::pair<std::string, Array>> in, out;

void read_blob(const std::string &path)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    auto get = [&](void *dst, size_t n) { if (n && std::fread(dst, 1, n, f) != n) throw std::runtime_error(path + ": truncated"); };
    uint32_t len;
    while (std::fread(&len, 1, 4, f) == 4)
    {
        std::string name(len, '\0');
        get(&name[0], len);
        Array a;
        uint32_t ndim;
        get(&a.dtype, 4); get(&ndim, 4);
        if (a.dtype > U32) throw std::runtime_error(path + ": a dtype this program does not read");
        a.dims.resize(ndim);
        get(a.dims.data(), 8 * (size_t)ndim);
        size_t count = 1;
        for (uint64_t d : a.dims) count *= (size_t)d;
        a.bytes.resize(count * 4);
        get(a.bytes.data(), a.bytes.size());
        in.emplace_back(std::move(name), std::move(a));
    }
    std::fclose(f);
}

void write_blob(const std::string &path)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot open " + path);
    for (const auto &it : out)
    {
        const uint32_t len = (uint32_t)it.first.size(), ndim = (uint32_t)it.second.dims.size();
        std::fwrite(&len, 4, 1, f); std::fwrite(it.first.data(), 1, len, f);
        std::fwrite(&it.second.dtype, 4, 1, f); std::fwrite(&ndim, 4, 1, f);
        std::fwrite(it.second.dims.data(), 8, ndim, f);
        std::fwrite(it.second.bytes.data(), 1, it.second.bytes.size(), f);
    }
    if (std::fclose(f) != 0) throw std::runtime_error("cannot write " + path);
}

const Array &at(const std::string &name, uint32_t dtype)
{
    for (const auto &it : in)
        if (it.first == name)
        {
            if (it.second.dtype != dtype) throw std::runtime_error("input " + name + " has another dtype");
            return it.second;
        }
    throw std::runtime_error("input " + name + " is missing");
}
const float *f32(const std::string &name) { return (const float *)at(name, F32).bytes.data(); }
const uint32_t *u32(const std::string &name) { return (const uint32_t *)at(name, U32).bytes.data(); }
float F(const std::string &name) { return f32(name)[0]; }
uint32_t U(const std::string &name) { return u32(name)[0]; }
void put(const std::string &name, uint32_t dtype, std::vector<uint64_t> dims, const void *data)
{
    Array a;
    a.dtype = dtype;
    a.dims = std::move(dims);
    size_t count = 1;
    for (uint64_t d : a.dims) count *= (size_t)d;
    a.bytes.assign((const uint8_t *)data, (const uint8_t *)data + count * 4);
    out.emplace_back(name, std::move(a));
}
void put_scalar(const std::string &name, uint32_t v) { put(name, U32, {1}, &v); }

// on the device: a Cornell-box mesh of two triangles gets a lightmap UV set that cuts it along its diagonal, and the atlas of
// the blob is stitched across that cut; then the refusals of the wrapper
void section_stitch_lightmap()
{
    const std::string k = "stitch_lightmap";
    lp::Device d(0);
    lp::Scene scene = lpl::build_scene_cornell_box(d).first;
    const uint32_t mesh = U(k + ".mesh_idx");
    const Array &uvs = at(k + ".uvs", F32);
    scene.set_lightmap_uvs(mesh, (const float *)uvs.bytes.data(), uvs.dims.at(0) * 3);
    lp::StitchDesc desc;
    desc.width = U(k + ".width");
    desc.height = U(k + ".height");
    desc.iterations = U(k + ".iterations");
    desc.samples_per_texel = F(k + ".samples_per_texel");
    desc.lambda = F(k + ".lam");
    lp::LightmapChart chart;
    chart.instance_idx = U(k + ".instance_idx");
    chart.scale_u = F(k + ".scale_u"); chart.scale_v = F(k + ".scale_v");
    chart.offset_u = F(k + ".offset_u"); chart.offset_v = F(k + ".offset_v");
    const lp::StitchResult r = lp::stitch_lightmap(d, scene, desc, &chart, 1, f32(k + ".rgba"));
    put(k + ".out", F32, {desc.height, desc.width, 4}, r.rgba.data());
    static_assert(sizeof(LupinLightmapStitchInfo) == 48, "the info is 12 words");
    put(k + ".info", U32, {12}, &r.info);
    const LupinLightmapStitchStats stats = lp::lightmap_stitch_stats();
    put_scalar(k + ".timed", stats.call_ms > 0.0f ? 1u : 0u);
    // the defaults of the descriptor are the Python host's
    const lp::StitchDesc def;
    const float defaults[3] = {(float)def.iterations, def.samples_per_texel, def.lambda};
    put(k + ".defaults", F32, {3}, defaults);
    // refusals: iterations above the maximum; a lambda of zero; device pointers without an output
    std::vector<uint32_t> refused;
    lp::StitchDesc bad[3] = {desc, desc, desc};
    bad[0].iterations = LUPIN_LIGHTMAP_STITCH_MAX_ITERATIONS + 1;
    bad[1].lambda = 0.0f;
    bad[2].flags = LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS;
    for (const lp::StitchDesc &b : bad)
    {
        try { lp::stitch_lightmap(d, scene, b, &chart, 1, f32(k + ".rgba")); refused.push_back(0); }
        catch (const lp::Error &e) { refused.push_back(e.code == LUPIN_ERR_INVALID_ARGUMENT ? 1u : 2u); }
    }
    put(k + ".refused", U32, {refused.size()}, refused.data());
}

struct Section { const char *name; const char *covers; void (*run)(); };
const Section SECTIONS[] = {
    {"stitch_lightmap", "stitch_lightmap lightmap_stitch_stats set_lightmap_uvs", section_stitch_lightmap},
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && std::string(argv[1]) == "--list")
    {
        for (const Section &s : SECTIONS) std::cout << s.name << ": " << s.covers << "\n";
        return 0;
    }
    if (argc < 3) { std::cerr << "usage: stitch_mirror_probe <inputs.bin> <outputs.bin> [section ...] | --list\n"; return 2; }
    std::string running = "reading the inputs";
    try
    {
        read_blob(argv[1]);
        for (const Section &s : SECTIONS)
        {
            bool wanted = argc == 3;
            for (int a = 3; a < argc; a++) wanted = wanted || std::string(argv[a]) == s.name;
            if (!wanted) continue;
            running = s.name;
            s.run();
            put_scalar(std::string("done.") + s.name, 1u);
        }
        write_blob(argv[2]);
    }
    catch (const std::exception &e)
    {
        std::cerr << running << ": " << e.what() << "\n";
        return 1;
    }
    return 0;
}
