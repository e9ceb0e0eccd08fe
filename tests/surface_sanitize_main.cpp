// Host driver for the surface-probe tests: runs oracle_surface_probe's TEXTURE mode over records read from a file, in a build
// with -fsanitize=address,undefined (the CPU test of tests/test_surface_probe.py compiles and runs it; the GPU test sends
// only the record set, pinned by a digest, that this run passed).
// File layout (little endian): u32 num_textures, u32 num_records; per texture u32 width, height, format and its texels;
// then the records (LUPIN_SURFACE_IN_FLOATS floats each).  Output file: LUPIN_SURFACE_OUT_FLOATS floats per record.
#include "../oracle/lupin_oracle.cpp"

#include <cstdio>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[2];
    if (fread(head, 4, 2, f) != 2) return 2;
    std::vector<std::vector<uint8_t>> texels(head[0]);
    std::vector<LupinTextureDesc> descs(head[0]);
    for (uint32_t i = 0; i < head[0]; i++)
    {
        uint32_t whf[3];
        if (fread(whf, 4, 3, f) != 3) return 2;
        const size_t bytes = (size_t)whf[0] * whf[1] * (whf[2] == LUPIN_TEX_RGBA8_UNORM ? 4 : 8);
        texels[i].resize(bytes);   // exactly the texture's size: a read past it is a heap overflow the sanitizer reports
        if (fread(texels[i].data(), 1, bytes, f) != bytes) return 2;
        memset(&descs[i], 0, sizeof(descs[i]));
        descs[i].width = whf[0]; descs[i].height = whf[1]; descs[i].format = whf[2]; descs[i].pixels = texels[i].data();
    }
    std::vector<float> rec((size_t)head[1] * LUPIN_SURFACE_IN_FLOATS), out((size_t)head[1] * LUPIN_SURFACE_OUT_FLOATS);
    if (fread(rec.data(), 4, rec.size(), f) != rec.size()) return 2;
    fclose(f);
    LupinSceneDesc scene;
    memset(&scene, 0, sizeof(scene));
    scene.textures = descs.data();
    scene.num_textures = head[0];
    const int rc = oracle_surface_probe(&scene, 0u, head[1], rec.data(), out.data());
    if (rc != 0) return 3;
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 2;
    fwrite(out.data(), 4, out.size(), g);
    fclose(g);
    return 0;
}
