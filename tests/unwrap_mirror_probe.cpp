// unwrap_mirror_probe.cpp -- runs the C++ host mirror of the lightmap UV sets (include/lupin_unwrap.hpp and
// lp::Scene::set_lightmap_uvs) on inputs read from a blob and writes every output to a blob; tests/test_unwrap_mirror.py makes
// the same calls through the Python host and compares the words.  The blob format is tests/cpp_mirror_probe.cpp's.
//
//   unwrap_mirror_probe <inputs.bin> <outputs.bin> [section ...]     no section names: every section
//   unwrap_mirror_probe --list                                       one line per section: its name, then the lp:: names it runs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "lupin_loader.hpp"
#include "lupin_unwrap.hpp"

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

void put_charts(const std::string &k, const std::vector<lp::LightmapChart> &charts)
{
    std::vector<uint32_t> inst;
    std::vector<float> so;
    for (const lp::LightmapChart &c : charts)
    {
        inst.push_back(c.instance_idx);
        so.insert(so.end(), {c.scale_u, c.scale_v, c.offset_u, c.offset_v});
    }
    put(k + ".instance_idx", U32, {charts.size()}, inst.data());
    put(k + ".scale_offset", F32, {charts.size(), 4}, so.data());
}

// host only: the placed charts, the atlas, and what is refused
void section_pack_lightmap_instances()
{
    const std::string k = "pack_lightmap_instances";
    const uint64_t n = at(k + ".sizes", U32).dims.at(0);
    const uint32_t *s = u32(k + ".sizes");
    const float *m = f32(k + ".multipliers");
    std::vector<std::pair<uint32_t, uint32_t>> sizes;
    for (uint64_t i = 0; i < n; i++) sizes.emplace_back(s[2 * i], s[2 * i + 1]);
    uint32_t W = 0, H = 0;
    const std::vector<lp::LightmapChart> charts = lp::pack_lightmap_instances(sizes, std::vector<float>(m, m + n), U(k + ".gutter"), &W, &H);
    put_charts(k + ".charts", charts);
    put_scalar(k + ".width", W);
    put_scalar(k + ".height", H);
    // refusals: a multiplier of zero; a size of zero; an entry above the largest atlas
    std::vector<uint32_t> refused;
    const std::pair<std::vector<std::pair<uint32_t, uint32_t>>, std::vector<float>> bad[3] = {
        {{{8u, 8u}}, {0.0f}}, {{{0u, 8u}}, {1.0f}}, {{{16000u, 8u}}, {2.0f}}};
    for (const auto &b : bad)
    {
        uint32_t w = 77, h = 77;
        try { lp::pack_lightmap_instances(b.first, b.second, 1, &w, &h); refused.push_back(0); }
        catch (const lp::Error &e) { refused.push_back(e.code == LUPIN_ERR_INVALID_ARGUMENT && w == 77 && h == 77 ? 1u : 2u); }
    }
    put(k + ".refused", U32, {refused.size()}, refused.data());
}

// on the device: the unwrap of one Cornell-box mesh, the set attached, a bake that reads it, the set removed
void section_unwrap_lightmap_uvs()
{
    const std::string k = "unwrap_lightmap_uvs";
    lp::Device d(0);
    lp::Scene scene = lpl::build_scene_cornell_box(d).first;
    lp::UnwrapDesc desc;
    desc.texel_size = F(k + ".texel_size");
    desc.padding = U(k + ".padding");
    const uint32_t mesh = U(k + ".mesh_idx");
    const lp::UnwrapResult r = lp::unwrap_lightmap_uvs(d, scene, mesh, desc);
    const uint32_t tris = (uint32_t)r.chart_of_tri.size();
    if (tris != U(k + ".num_tris") || r.uvs.size() != (size_t)tris * 6) throw std::runtime_error("the wrapper sized its outputs by another triangle count");
    put(k + ".uvs", F32, {tris, 3, 2}, r.uvs.data());
    put(k + ".chart_of_tri", U32, {tris}, r.chart_of_tri.data());
    const uint32_t info[4] = {r.info.num_charts, r.info.width, r.info.height, r.info.degenerate_tris};
    put(k + ".info", U32, {4}, info);

    scene.set_lightmap_uvs(mesh, r.uvs.data(), (uint64_t)tris * 3);
    uint32_t W = 0, H = 0;
    std::vector<lp::LightmapChart> charts = lp::pack_lightmap_instances({{r.info.width, r.info.height}}, {F(k + ".multiplier")}, U(k + ".gutter"), &W, &H);
    charts[0].instance_idx = U(k + ".instance_idx");
    lp::LightmapDesc ld;
    ld.width = W; ld.height = H;
    ld.samples = U(k + ".samples");
    ld.max_bounces = U(k + ".max_bounces");
    ld.counter = U(k + ".counter");
    ld.surface_offset = F(k + ".surface_offset");
    std::vector<float> rgba((size_t)W * H * 4), records((size_t)W * H * 8);
    const uint64_t covered = lp::bake_lightmap(d, scene, ld, charts.data(), 1, rgba.data(), records.data());
    put(k + ".rgba", F32, {H, W, 4}, rgba.data());
    put(k + ".records", F32, {H, W, 8}, records.data());
    put_scalar(k + ".covered", (uint32_t)covered);

    scene.set_lightmap_uvs(mesh, nullptr, 0);      // removed: the mesh has no texcoords either, so the bake is refused again
    uint32_t refused = 0;
    try { lp::bake_lightmap(d, scene, ld, charts.data(), 1, rgba.data()); }
    catch (const lp::Error &e) { refused = e.code == LUPIN_ERR_INVALID_ARGUMENT ? 1u : 2u; }
    put_scalar(k + ".refused_without_a_set", refused);
}

struct Section { const char *name; const char *covers; void (*run)(); };
const Section SECTIONS[] = {
    {"pack_lightmap_instances", "pack_lightmap_instances", section_pack_lightmap_instances},
    {"unwrap_lightmap_uvs", "unwrap_lightmap_uvs set_lightmap_uvs pack_lightmap_instances bake_lightmap", section_unwrap_lightmap_uvs},
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && std::string(argv[1]) == "--list")
    {
        for (const Section &s : SECTIONS) std::cout << s.name << ": " << s.covers << "\n";
        return 0;
    }
    if (argc < 3) { std::cerr << "usage: unwrap_mirror_probe <inputs.bin> <outputs.bin> [section ...] | --list\n"; return 2; }
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
