// ORACLE TOOLING — builds ONLY in a container that has /root/reference; output goes to oracle/_ref/.
// Harness around the reference's own hw8 scene.cpp, compiled where it lies and unmodified: it is included textually (found through
// -I$(REF)/hw8/src), so that its static functions sampleTexture and applyNormalMaps can be called, next to primitives.cpp and
// color.cpp.  Its one third-party include is answered by standin/stb_image.h.  The whole hw8 integrator (Scene::getPixel -> getColor
// with textures, normal maps and the environment map) runs as the reference wrote it; only the glTF loader (sceneio.cpp, which
// needs the absent rapidjson and the image decoders) is replaced by filling Scene's public members from an rt_scene_desc.
#include "scene.cpp"
#include "../../include/rtamd.h"
#include <omp.h>
#include <cstdlib>
#include <cstring>

extern "C" void stbi_image_free(void *p) { free(p); }

namespace {
Vec3 v3(const float *p) { return Vec3(p[0], p[1], p[2]); }
// The harness's own copy of an image, freed by Scene::~Scene through stbi_image_free.  Behind the last texel lie 3 * (width + 1) zero
// bytes: when a wrapped coordinate times the size rounds up to the size itself, loadSingleFromTexture reads texel (width, iy) or row
// `height`, at most 3 * (width + width * height) + 2 bytes from the start.  With the zeros that read is defined, and it is the 0 that
// the oracle and the device define for a texel past the end.
Texture copy_image(int w, int h, const uint8_t *rgb) {
    const size_t bytes = (size_t)3 * w * h, pad = (size_t)3 * (w + 1);
    uint8_t *data = (uint8_t *)malloc(bytes + pad);
    memcpy(data, rgb, bytes);
    memset(data + bytes, 0, pad);
    return Texture{w, h, data};
}
std::optional<size_t> opt(int32_t t) { return t >= 0 ? std::optional<size_t>((size_t)t) : std::nullopt; }
}

extern "C" {
#pragma GCC visibility push(default)
void *ref8s_create(const rt_scene_desc *d) {
    Scene *s = new Scene();
    for (uint32_t i = 0; i < d->n_materials; i++) {
        const rt_material &m = d->materials[i];
        GltfMaterial g;
        g.color = v3(m.base_color);
        g.emission = v3(m.emission);
        g.metallicFactor = m.metallic_factor;
        g.roughnessFactor = m.roughness_factor;
        g.baseColorTexture = opt(m.base_color_texture);
        g.emissiveTexture = opt(m.emissive_texture);
        g.metallicRoughnessTexture = opt(m.metallic_roughness_texture);
        g.normalTexture = opt(m.normal_texture);
        s->materials.push_back(g);
        s->materialModels.push_back(MaterialModel(g.metallicFactor, g.color)); // hw8/src/sceneio.cpp:239-244
    }
    for (uint32_t i = 0; i < d->n_textures; i++) s->textureDescs.push_back(TextureDesc{0, d->texture_source[i]});
    for (uint32_t i = 0; i < d->n_images; i++) s->textureImages.push_back(copy_image(d->images[i].width, d->images[i].height, d->images[i].rgb));
    if (d->environment_map) s->environmentMap = copy_image(d->environment_map->width, d->environment_map->height, d->environment_map->rgb);
    for (uint32_t i = 0; i < d->n_triangles; i++) {
        Vertex vs[3];
        for (int k = 0; k < 3; k++) {
            vs[k] = Vertex(v3(d->positions + 9 * i + 3 * k),
                           Vec2(d->texcoords[6 * i + 2 * k], d->texcoords[6 * i + 2 * k + 1]),
                           v3(d->normals + 9 * i + 3 * k),
                           Vec4(v3(d->tangents + 12 * i + 4 * k), d->tangents[12 * i + 4 * k + 3]));
        }
        Figure f(vs[0], vs[1], vs[2]);
        f.materialIndex = d->material_index[i];
        f.material = s->materials[f.materialIndex];
        s->figures.push_back(f);
    }
    s->cameraPos = v3(d->camera.position); s->cameraRight = v3(d->camera.right);
    s->cameraUp = v3(d->camera.up); s->cameraForward = v3(d->camera.forward);
    s->cameraFovY = d->camera.fov_y;
    s->bgColor = v3(d->bg_color);
    s->initBVH();
    s->initDistribution();
    return s;
}
void ref8s_destroy(void *p) { delete (Scene *)p; }
// Pixel rectangle of the reference's render loop, the engine of pixel (x, y) seeded y * width + x.
int ref8s_render(void *p, int width, int height, int samples, int ray_depth, int x0, int y0, int w, int h, float *out_rgb, uint8_t *out8, int nthreads) {
    Scene *s = (Scene *)p;
    s->width = width; s->height = height; s->samples = samples; s->rayDepth = ray_depth > 0 ? ray_depth : 6;
    if (nthreads <= 0) nthreads = omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 8) num_threads(nthreads)
    for (int j = 0; j < w * h; j++) {
        int x = x0 + j % w, y = y0 + j / w;
        rng_type rng(y * width + x);
        Color px = s->getPixel(rng, x, y);
        if (out_rgb) { out_rgb[3 * j] = px.x; out_rgb[3 * j + 1] = px.y; out_rgb[3 * j + 2] = px.z; }
        if (out8) { auto a = toExternColorFormat(gamma_corrected(aces_tonemap(px))); out8[3 * j] = a[0]; out8[3 * j + 1] = a[1]; out8[3 * j + 2] = a[2]; }
    }
    return 0;
}
// scene.cpp's static sampleTexture on one tap of an image (on a padded copy, as above).
void ref8_sample_texture(int w, int h, const uint8_t *data, float tx, float ty, int srgb, float *out3) {
    Texture t = copy_image(w, h, data);
    Vec3 r = sampleTexture(tx, ty, t, srgb != 0);
    out3[0] = r.x; out3[1] = r.y; out3[2] = r.z;
    free(t.data);
}
// scene.cpp's static applyNormalMaps: the shading normal, the tangent (xyz, w) and the normal map's tap.
void ref8_apply_normal_map(const float *sn3, const float *tan4, const float *sample3, float *out3) {
    Vec3 r = applyNormalMaps(v3(sn3), Vec4(v3(tan4), tan4[3]), v3(sample3), false);
    out3[0] = r.x; out3[1] = r.y; out3[2] = r.z;
}
#pragma GCC visibility pop
}
