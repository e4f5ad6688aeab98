// CLI with the reference's surfaces:
//   hw6-hw8 (hw8/src/main.cpp:7-18, hw8/run.sh):  rtamd_main <scene.gltf> <width> <height> <samples> <out.ppm> [<envmap.png>]
//   hw1-hw5 (hw1/src/main.cpp:7-14, hw1/run.sh):  rtamd_main <scene.txt> <out.ppm>
// Which snapshot's integrator replays the scene: RTAMD_SNAPSHOT=hw8 (default for glTF) | hw7 | hw6, and for .txt scenes
// hw1 | hw2 | hw3 (default) | hw4 | hw5 (grammar and integrator of that snapshot).
// The host only parses, prepares and writes the PPM; the render loop runs on the GPU through the C-ABI — on EVERY visible GPU
// when there are several (rt_multi_*: tiles dealt round-robin, one exchange step to the first device; RTAMD_DEVICES=n limits
// the count, RTAMD_DEVICES=1 forces the single-device path; RTAMD_DEVICE_LIST=0,0,1 names the HIP devices of rt_multi_create itself,
// repeats allowed).
// Progressive renders of the glTF surface (rt_accum_* on one device, rt_multi_accum_* on several: the checkpoint file is the same
// either way, so a frame begun on eight GPUs can be finished on one): RTAMD_SLICE=n renders in slices of n samples and rewrites the PPM
// after every slice; RTAMD_CHECKPOINT=path carries on from that file when it exists and writes it after every slice (both files are
// written under a temporary name and renamed, so a reader never sees half a file); RTAMD_SLICE_LIMIT=k stops after k slices.
// Stopping at a noise target (rt_noise_* / rt_multi_noise_*, which only read the frame in progress): RTAMD_TARGET_NOISE=x renders in slices
// (of RTAMD_SLICE samples, else a sixteenth of the samples asked for), prints the estimated noise of the picture (RMS error of its luminance
// over its mean luminance) after every slice from the second on and ends the run at the first slice where it is at most x, once
// RTAMD_NOISE_MIN_BATCHES slices (default 4, at least 2) have been observed: the file is then the plain run's at that many samples.
// RTAMD_NOISE_MAP=path writes the last per-pixel standard error as a grayscale PFM ("Pf", little-endian, bottom row first as PFM has it).
// First-hit guide images for a denoiser (rt_render_guides, glTF surface, hw8 / hw7): RTAMD_GUIDES=prefix writes prefix_albedo.pfm and
// prefix_normal.pfm ("PF") and prefix_depth.pfm ("Pf") at the frame's size before the frame is rendered; out.ppm is the run's without it.
// Denoised previews (rt_accum_denoise, glTF surface, hw8 / hw7): RTAMD_DENOISE=path.ppm writes the filtered picture next to out.ppm, in a
// sliced run after every slice, steered by the noise monitor's error map whenever a monitor runs (RTAMD_TARGET_NOISE, RTAMD_NOISE_MAP) and
// has two batches; RTAMD_DENOISE_ALBEDO=1 demodulates by the albedo plane.  out.ppm is the run's without it.  With several devices the
// frame and the map come to the host (rt_multi_accum_resolve, rt_multi_noise_estimate) and rt_denoise filters them on a scene of its own.
// Adaptive sampling (rt_adaptive_*, glTF surface, hw8, one GPU): RTAMD_ADAPTIVE=1 together with RTAMD_TARGET_NOISE=x renders in slices of
// RTAMD_SLICE samples (else a sixteenth of the samples asked for) and stops drawing samples for every 8x8 sub-tile whose own noise is at
// most x times the frame's mean luminance, once RTAMD_NOISE_MIN_BATCHES slices of it have been observed; the samples asked for are the
// most any sub-tile draws.  RTAMD_ADAPTIVE_DILATE=1 keeps the neighbours of an unfinished sub-tile drawing.  After every slice one line
// on stderr: the sub-tiles that drew, the converged and the capped ones, the frame's noise.  RTAMD_SAMPLE_MAP=path writes the samples per
// pixel as a grayscale PFM.  out.ppm is rt_adaptive_resolve's bytes: every sub-tile the plain run's picture at that sub-tile's count.
// On several GPUs, with another snapshot or with a checkpoint the run ends with an error that names the reason.
// A batch of cameras (rt_views_*, glTF surface, hw8, one GPU): RTAMD_CAMERAS=file gives one camera per line as 13 floats -- position,
// right, up, forward, fov_y; empty lines and lines that begin with # are skipped.  The run renders all of them as one view set from the
// one scene, in one slice or with RTAMD_SLICE in slices of that many samples, and writes out_000.ppm, out_001.ppm, ... beside the named
// output (its name before the extension, then the camera's number).  A malformed line ends the run with RT_ERR_PARSE and names the line.
// Both together (rt_view_adaptive_*): RTAMD_CAMERAS=file with RTAMD_ADAPTIVE=1 and RTAMD_TARGET_NOISE=x renders the file's cameras as one
// adaptive set in slices of RTAMD_SLICE (else a sixteenth of the samples asked for, which are the most any sub-tile draws) until no
// sub-tile of any view is active, each view judged by its own mean luminance.  After every slice one line on stderr: the views and
// sub-tiles that drew, the converged and the capped sub-tiles.  It writes out_000.ppm, ... and, with RTAMD_SAMPLE_MAP=spp.pfm,
// spp_000.pfm, ...; RTAMD_ADAPTIVE_DILATE is honoured.
#include "../../../include/rtamd.h"
#include "../host/knobs.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int die() {
    fprintf(stderr, "error: %s\n", rt_last_error());
    return 1;
}

static bool write_file_atomically(const std::string &path, const void *data, size_t size) {
    const std::string tmp = path + ".part";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(data, 1, size, f) == size;
    if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path.c_str()) != 0) { remove(tmp.c_str()); return false; }
    return true;
}

// A frame in progress: an rt_accum on one device or an rt_multi_accum on all of them, the same calls either way.
struct Progress {
    rt_accum *one = nullptr;
    rt_multi_accum *all = nullptr;
    int samples() const { return all ? rt_multi_accum_samples(all) : rt_accum_samples(one); }
    int render(int n, rt_stats *st) { return all ? rt_multi_accum_render(all, n, st) : rt_accum_render(one, n, st); }
    int resolve(uint8_t *rgb8) { return all ? rt_multi_accum_resolve(all, 0, nullptr, rgb8) : rt_accum_resolve(one, 0, nullptr, rgb8); }
    int save(void *blob, size_t capacity) { return all ? rt_multi_accum_save(all, blob, capacity) : rt_accum_save(one, blob, capacity); }
    int load(const void *blob, size_t size) { return all ? rt_multi_accum_load(all, blob, size) : rt_accum_load(one, blob, size); }
    void destroy() { if (all) rt_multi_accum_destroy(all); else rt_accum_destroy(one); all = nullptr; one = nullptr; }
};

// The noise monitor of a frame in progress, on whichever of the two it is.
struct Monitor {
    rt_noise *one = nullptr;
    rt_multi_noise *all = nullptr;
    int create(Progress &acc) { return acc.all ? rt_multi_noise_create(acc.all, &all) : rt_noise_create(acc.one, &one); }
    int update() { return all ? rt_multi_noise_update(all) : rt_noise_update(one); }
    int batches() const { return all ? rt_multi_noise_batches(all) : rt_noise_batches(one); }
    int estimate(float *se, rt_noise_summary *s) { return all ? rt_multi_noise_estimate(all, 0, se, s) : rt_noise_estimate(one, 0, se, s); }
    void destroy() { if (all) rt_multi_noise_destroy(all); else if (one) rt_noise_destroy(one); all = nullptr; one = nullptr; }
};
struct NoiseTarget {
    double target = 0;           // RTAMD_TARGET_NOISE, 0 = none
    int min_batches = 4;         // RTAMD_NOISE_MIN_BATCHES
    const char *map = nullptr;   // RTAMD_NOISE_MAP
    bool active() const { return target > 0 || map; }
};

// A float image (row 0 first) as a PFM: "Pf" for one channel, "PF" for three; a negative scale = little-endian floats, rows from the bottom up.
static bool write_pfm(const std::string &path, int width, int height, int channels, const std::vector<float> &image) {
    char head[64];
    const int n = snprintf(head, sizeof head, "%s\n%d %d\n-1.0\n", channels == 3 ? "PF" : "Pf", width, height);
    const size_t row = (size_t)width * channels;
    std::vector<uint8_t> file((size_t)n + image.size() * sizeof(float));
    memcpy(file.data(), head, (size_t)n);
    for (int y = 0; y < height; y++) memcpy(file.data() + n + (size_t)y * row * sizeof(float), image.data() + (size_t)(height - 1 - y) * row, row * sizeof(float));
    return write_file_atomically(path, file.data(), file.size());
}

// RTAMD_GUIDES=prefix: the first-hit guide images of the frame (rt_render_guides) as prefix_albedo.pfm, prefix_normal.pfm, prefix_depth.pfm.
static int write_guides(rt_scene *scene, const rt_render_params &p, const std::string &prefix) {
    const size_t px = (size_t)p.width * p.height;
    std::vector<float> albedo(px * 3), normal(px * 3), depth(px);
    rt_query_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    if (rt_render_guides(scene, p.width, p.height, 0, albedo.data(), normal.data(), depth.data(), nullptr, &st) != RT_OK) return die();
    fprintf(stderr, "guides: %.3f ms on the GPU in %u launches\n", st.kernel_ms, st.launches);
    const struct { const char *name; int channels; const std::vector<float> &image; } planes[] = {{"_albedo.pfm", 3, albedo}, {"_normal.pfm", 3, normal}, {"_depth.pfm", 1, depth}};
    for (const auto &pl : planes)
        if (!write_pfm(prefix + pl.name, p.width, p.height, pl.channels, pl.image)) { fprintf(stderr, "error: cannot write guide image %s%s\n", prefix.c_str(), pl.name); return 1; }
    return 0;
}

// RTAMD_DENOISE=path: the filtered preview of the picture so far.  On one device rt_accum_denoise composes it on the GPU; on several the
// frame and the error map come to the host and rt_denoise filters them on `scene`, a scene of the preview's own on the current device,
// with the frame's guide planes made there once.
struct Preview {
    const char *path = nullptr;  // RTAMD_DENOISE
    bool albedo = false;         // RTAMD_DENOISE_ALBEDO=1
    rt_scene *scene = nullptr;   // several devices only
    std::vector<float> guides;   // several devices only: albedo, normal, depth, emission
};
static int write_preview(Preview &pv, Progress &acc, Monitor &mon, bool monitored, const rt_render_params &p, std::vector<uint8_t> &rgb8) {
    rt_denoise_params dp;
    memset(&dp, 0, sizeof dp);
    dp.struct_size = sizeof dp;
    const bool with_map = monitored && mon.batches() >= 2;
    const size_t px = (size_t)p.width * p.height;
    if (acc.one) {
        dp.flags = pv.albedo ? RT_DENOISE_ALBEDO : 0u;
        if (rt_accum_denoise(acc.one, with_map ? mon.one : nullptr, &dp, nullptr, rgb8.data(), nullptr) != RT_OK) return die();
    } else {
        if (pv.guides.empty()) {
            pv.guides.resize(px * 10);
            float *g = pv.guides.data();
            if (rt_render_guides(pv.scene, p.width, p.height, 0, g, g + 3 * px, g + 6 * px, g + 7 * px, nullptr) != RT_OK) return die();
        }
        std::vector<float> rgb(px * 3), se(with_map ? px : 0);
        if (rt_multi_accum_resolve(acc.all, 0, rgb.data(), nullptr) != RT_OK) return die();
        if (with_map && rt_multi_noise_estimate(mon.all, 0, se.data(), nullptr) != RT_OK) return die();
        const float *g = pv.guides.data();
        dp.width = p.width; dp.height = p.height;
        if (rt_denoise(pv.scene, &dp, rgb.data(), g + 3 * px, g + 6 * px, pv.albedo ? g : nullptr, g + 7 * px, with_map ? se.data() : nullptr, nullptr, rgb8.data(), nullptr) != RT_OK) return die();
    }
    const std::string tmp = std::string(pv.path) + ".part";
    if (rt_write_ppm(tmp.c_str(), p.width, p.height, rgb8.data()) != RT_OK) return die();
    if (rename(tmp.c_str(), pv.path) != 0) { fprintf(stderr, "error: cannot rename %s to %s\n", tmp.c_str(), pv.path); return 1; }
    return 0;
}

// The frame in slices: the picture after every slice is the frame of that many samples, the last one the frame of the plain run.
// `p` are the params of the unsharded frame, whose rt_accum_state_bytes is the size of the checkpoint on any number of devices.
// With a noise target the run ends at the first slice whose picture is quiet enough: that picture is the plain run's at that many samples.
static int render_in_slices(Progress &acc, const rt_render_params &p, int slice, const char *checkpoint, const char *out_path, std::vector<uint8_t> &rgb8, const NoiseTarget &noise, Preview &preview) {
    std::vector<uint8_t> blob(checkpoint ? rt_accum_state_bytes(&p) : 0);
    if (checkpoint) {
        if (FILE *f = fopen(checkpoint, "rb")) {
            std::vector<uint8_t> in(blob.size() + 1);
            const size_t got = fread(in.data(), 1, in.size(), f);
            fclose(f);
            if (acc.load(in.data(), got) != RT_OK) { fprintf(stderr, "error: checkpoint %s does not match this command line: %s\n", checkpoint, rt_last_error()); return 1; }
            if (got != blob.size()) { fprintf(stderr, "error: checkpoint %s has %zu bytes where this frame's has %zu\n", checkpoint, got, blob.size()); return 1; }
            if (acc.samples() > p.samples) { fprintf(stderr, "error: checkpoint %s holds %d samples, more than the %d asked for\n", checkpoint, acc.samples(), p.samples); return 1; }
            fprintf(stderr, "checkpoint: %s loaded, %d of %d samples done\n", checkpoint, acc.samples(), p.samples);
        }
    }
    Monitor mon; // after the checkpoint: its batches start at the state that was loaded
    if (noise.active() && mon.create(acc) != RT_OK) return die();
    // the monitor goes before the frame it watches; with RTAMD_NOISE_MAP its last map is written first
    auto end_monitor = [&]() -> int {
        int rc = 0;
        if (noise.map && mon.batches() >= 2) {
            std::vector<float> se((size_t)p.width * p.height);
            if (mon.estimate(se.data(), nullptr) != RT_OK) rc = die();
            else if (!write_pfm(noise.map, p.width, p.height, 1, se)) { fprintf(stderr, "error: cannot write noise map %s\n", noise.map); rc = 1; }
        } else if (noise.map) {
            fprintf(stderr, "note: no noise map written: the estimate needs two slices of this run\n");
        }
        mon.destroy();
        return rc;
    };
    const int limit = getenv("RTAMD_SLICE_LIMIT") ? atoi(getenv("RTAMD_SLICE_LIMIT")) : 0;
    const std::string tmp_ppm = std::string(out_path) + ".part";
    double kernel_ms = 0;
    uint64_t samples = 0;
    uint32_t exact = 1;
    bool converged = false;
    for (int k = 0;; k++) {
        const int done = acc.samples();
        if (k > 0 || done == p.samples) { // the picture so far (a checkpoint that already holds the frame just resolves)
            if (acc.resolve(rgb8.data()) != RT_OK) return die();
            if (rt_write_ppm(tmp_ppm.c_str(), p.width, p.height, rgb8.data()) != RT_OK) return die();
            if (rename(tmp_ppm.c_str(), out_path) != 0) { fprintf(stderr, "error: cannot rename %s to %s\n", tmp_ppm.c_str(), out_path); return 1; }
            if (preview.path) if (const int rc = write_preview(preview, acc, mon, noise.active(), p, rgb8)) return rc;
        }
        if (converged) fprintf(stderr, "CONVERGED after %d slices at %d of %d samples\n", k, done, p.samples);
        if (done == p.samples || converged) break;
        if (limit > 0 && k >= limit) {
            fprintf(stderr, "STOPPED after %d slices at %d of %d samples\n", k, done, p.samples);
            const int rc = end_monitor();
            acc.destroy();
            return rc ? rc : -1;
        }
        const int n = slice > 0 && slice < p.samples - done ? slice : p.samples - done;
        rt_stats st;
        if (acc.render(n, &st) != RT_OK) return die();
        kernel_ms += st.kernel_ms; samples += st.samples; exact &= st.reference_exact;
        fprintf(stderr, "slice %d: %d samples (%d of %d), %.3f ms on the GPU", k + 1, n, done + n, p.samples, st.kernel_ms);
        if (noise.active()) {
            if (mon.update() != RT_OK) { fprintf(stderr, "\n"); return die(); }
            if (mon.batches() >= 2) {
                rt_noise_summary ns;
                memset(&ns, 0, sizeof ns);
                ns.struct_size = sizeof ns;
                if (mon.estimate(nullptr, &ns) != RT_OK) { fprintf(stderr, "\n"); return die(); }
                fprintf(stderr, ", noise %.9g worst tile %.9g", ns.noise, ns.worst_tile_noise);
                converged = noise.target > 0 && mon.batches() >= noise.min_batches && ns.noise <= noise.target;
            }
        }
        fprintf(stderr, "\n");
        if (checkpoint) {
            if (acc.save(blob.data(), blob.size()) != RT_OK) return die();
            if (!write_file_atomically(checkpoint, blob.data(), blob.size())) { fprintf(stderr, "error: cannot write checkpoint %s\n", checkpoint); return 1; }
        }
    }
    if (samples) fprintf(stderr, "render: %.3f ms on the GPU, %.2f Msamples/s\n", kernel_ms, samples / (kernel_ms * 1e3));
    if (samples && !exact)
        fprintf(stderr, "note: this render kept the answers of the walkers' padded boxes (no exactness gate on this path: see rt_stats.reference_exact in rtamd.h); about one pixel in 1e5 may differ from the reference's\n");
    const int rc = end_monitor();
    acc.destroy();
    return rc;
}

// RTAMD_ADAPTIVE=1: slices of the policy until no sub-tile is active.
static int render_adaptive(rt_scene *scene, const rt_render_params &p, int slice, const NoiseTarget &noise, const char *out_path, std::vector<uint8_t> &rgb8) {
    rt_adaptive_params ap;
    memset(&ap, 0, sizeof ap);
    ap.struct_size = sizeof ap;
    ap.target_noise = (float)noise.target; ap.min_batches = noise.min_batches; ap.max_samples = p.samples;
    if (const char *e = getenv("RTAMD_ADAPTIVE_DILATE")) if (atoi(e) != 0) ap.flags |= RT_ADAPTIVE_DILATE;
    rt_render_params q = p;
    q.samples = 0;
    rt_adaptive *ad = nullptr;
    if (rt_adaptive_create(scene, &q, &ap, &ad) != RT_OK) return die();
    auto fail = [&]() { const int rc = die(); rt_adaptive_destroy(ad); return rc; };
    double kernel_ms = 0;
    uint64_t samples = 0;
    for (int k = 1;; k++) {
        rt_adaptive_stats st;
        memset(&st, 0, sizeof st);
        st.struct_size = sizeof st;
        if (rt_adaptive_render(ad, slice, &st) != RT_OK) return fail();
        if (st.samples == 0) break;
        kernel_ms += st.kernel_ms; samples += st.samples;
        fprintf(stderr, "slice %d: %u sub-tiles drew %d samples, %u converged, %u capped, %d .. %d samples per pixel, %.3f ms on the GPU", k, st.active_tiles, slice,
                st.converged_tiles, st.capped_tiles, st.min_samples, st.max_samples, st.kernel_ms);
        if (k >= 2) {
            rt_noise_summary ns;
            memset(&ns, 0, sizeof ns);
            ns.struct_size = sizeof ns;
            if (rt_adaptive_noise(ad, 0, nullptr, &ns) != RT_OK) { fprintf(stderr, "\n"); return fail(); }
            fprintf(stderr, ", noise %.9g worst tile %.9g", ns.noise, ns.worst_tile_noise);
        }
        fprintf(stderr, "\n");
    }
    if (samples) fprintf(stderr, "render: %.3f ms on the GPU, %.2f Msamples/s, %llu camera samples of the %llu a uniform run draws\n", kernel_ms, samples / (kernel_ms * 1e3),
                         (unsigned long long)samples, (unsigned long long)p.width * p.height * p.samples);
    if (rt_adaptive_resolve(ad, 0, nullptr, rgb8.data()) != RT_OK) return fail();
    if (const char *path = getenv("RTAMD_SAMPLE_MAP")) {
        std::vector<int32_t> spp((size_t)p.width * p.height);
        if (rt_adaptive_sample_map(ad, spp.data()) != RT_OK) return fail();
        const std::vector<float> image(spp.begin(), spp.end());
        if (!write_pfm(path, p.width, p.height, 1, image)) { fprintf(stderr, "error: cannot write sample map %s\n", path); rt_adaptive_destroy(ad); return 1; }
    }
    rt_adaptive_destroy(ad);
    if (rt_write_ppm(out_path, p.width, p.height, rgb8.data()) != RT_OK) return die();
    return 0;
}

// RTAMD_CAMERAS: the file's cameras, one per line; false (and the message printed) for a file that cannot be read or a malformed line.
static bool read_cameras(const char *path, std::vector<rt_camera> &cameras) {
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "error: RTAMD_CAMERAS: cannot open %s\n", path); return false; }
    char line[1024];
    for (int number = 1; fgets(line, sizeof line, f); number++) {
        const char *c = line + strspn(line, " \t\r\n");
        if (*c == 0 || *c == '#') continue;
        float v[13];
        int n = 0;
        for (; n < 13; n++) {
            char *end = nullptr;
            v[n] = strtof(c, &end);
            if (end == c) break;
            c = end;
        }
        if (n < 13 || c[strspn(c, " \t\r\n")] != 0) {
            fprintf(stderr, "error: RTAMD_CAMERAS: %s line %d: a camera is 13 numbers (position, right, up, forward, fov_y) and nothing else (RT_ERR_PARSE, %d)\n", path, number, (int)RT_ERR_PARSE);
            fclose(f);
            return false;
        }
        rt_camera cam;
        memset(&cam, 0, sizeof cam);
        for (int k = 0; k < 3; k++) { cam.position[k] = v[k]; cam.right[k] = v[3 + k]; cam.up[k] = v[6 + k]; cam.forward[k] = v[9 + k]; }
        cam.fov_y = v[12];
        cameras.push_back(cam);
    }
    fclose(f);
    if (cameras.empty()) { fprintf(stderr, "error: RTAMD_CAMERAS: %s holds no camera\n", path); return false; }
    return true;
}

// The file of view v beside `path`: out.ppm -> out_007.ppm (the extension, if any, is replaced by `ext`).
static std::string numbered(const char *path, size_t v, const char *ext) {
    std::string stem = path;
    const size_t dot = stem.rfind('.'), slash = stem.find_last_of('/');
    if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) stem.resize(dot);
    char tail[32];
    snprintf(tail, sizeof tail, "_%03zu", v);
    return stem + tail + ext;
}

// RTAMD_CAMERAS=file: all cameras as one view set, p.samples samples each in slices of `slice` (0: one slice), one PPM per camera.
static int render_views(rt_scene *scene, const rt_render_params &p, int slice, const std::vector<rt_camera> &cameras, const char *out_path, std::vector<uint8_t> &rgb8) {
    rt_views_params vp;
    memset(&vp, 0, sizeof vp);
    vp.struct_size = sizeof vp;
    vp.width = p.width; vp.height = p.height; vp.ray_depth = p.ray_depth; vp.n_views = (int32_t)cameras.size();
    rt_views *views = nullptr;
    if (rt_views_create(scene, &vp, cameras.data(), &views) != RT_OK) return die();
    auto fail = [&]() { const int rc = die(); rt_views_destroy(views); return rc; };
    double kernel_ms = 0;
    uint64_t samples = 0;
    for (int done = 0; done < p.samples;) {
        const int n = slice > 0 && slice < p.samples - done ? slice : p.samples - done;
        rt_views_stats st;
        memset(&st, 0, sizeof st);
        st.struct_size = sizeof st;
        if (rt_views_render(views, n, nullptr, &st) != RT_OK) return fail();
        done += n; kernel_ms += st.kernel_ms; samples += st.samples;
        if (slice > 0) fprintf(stderr, "slice: %u views drew %d samples, %d of %d, %.3f ms on the GPU, %llu first rays and bounces by the exact role\n", st.active_views, n, done, p.samples,
                               st.kernel_ms, (unsigned long long)st.exact_walks);
    }
    fprintf(stderr, "render: %zu views, %.3f ms on the GPU, %.2f Msamples/s\n", cameras.size(), kernel_ms, samples / (kernel_ms * 1e3));
    for (size_t v = 0; v < cameras.size(); v++) {
        if (rt_views_resolve(views, (int32_t)v, 0, nullptr, rgb8.data()) != RT_OK) return fail();
        if (rt_write_ppm(numbered(out_path, v, ".ppm").c_str(), p.width, p.height, rgb8.data()) != RT_OK) return fail();
    }
    rt_views_destroy(views);
    return 0;
}

// RTAMD_CAMERAS=file with RTAMD_ADAPTIVE=1: all cameras as one adaptive view set, slices of the policy until no sub-tile of any view is
// active; one PPM per camera and, with RTAMD_SAMPLE_MAP=spp.pfm, spp_000.pfm, ... beside it.
static int render_view_adaptive(rt_scene *scene, const rt_render_params &p, int slice, const NoiseTarget &noise, const std::vector<rt_camera> &cameras, const char *out_path,
                                std::vector<uint8_t> &rgb8) {
    rt_views_params vp;
    memset(&vp, 0, sizeof vp);
    vp.struct_size = sizeof vp;
    vp.width = p.width; vp.height = p.height; vp.ray_depth = p.ray_depth; vp.n_views = (int32_t)cameras.size();
    rt_adaptive_params ap;
    memset(&ap, 0, sizeof ap);
    ap.struct_size = sizeof ap;
    ap.target_noise = (float)noise.target; ap.min_batches = noise.min_batches; ap.max_samples = p.samples;
    if (const char *e = getenv("RTAMD_ADAPTIVE_DILATE")) if (atoi(e) != 0) ap.flags |= RT_ADAPTIVE_DILATE;
    rt_view_adaptive *set = nullptr;
    if (rt_view_adaptive_create(scene, &vp, &ap, cameras.data(), &set) != RT_OK) return die();
    auto fail = [&]() { const int rc = die(); rt_view_adaptive_destroy(set); return rc; };
    double kernel_ms = 0;
    uint64_t samples = 0;
    for (int k = 1;; k++) {
        rt_view_adaptive_stats st;
        memset(&st, 0, sizeof st);
        st.struct_size = sizeof st;
        if (rt_view_adaptive_render(set, slice, nullptr, &st) != RT_OK) return fail();
        if (st.samples == 0) break;
        kernel_ms += st.kernel_ms; samples += st.samples;
        fprintf(stderr, "slice %d: %u views, %u sub-tiles drew %d samples, %u converged, %u capped, %d .. %d samples per pixel, %.3f ms on the GPU\n", k, st.active_views, st.active_tiles,
                slice, st.converged_tiles, st.capped_tiles, st.min_samples, st.max_samples, st.kernel_ms);
    }
    if (samples) fprintf(stderr, "render: %zu views, %.3f ms on the GPU, %.2f Msamples/s, %llu camera samples of the %llu a uniform run draws\n", cameras.size(), kernel_ms,
                         samples / (kernel_ms * 1e3), (unsigned long long)samples, (unsigned long long)cameras.size() * p.width * p.height * p.samples);
    const char *map_path = getenv("RTAMD_SAMPLE_MAP");
    std::vector<int32_t> spp((size_t)p.width * p.height);
    for (size_t v = 0; v < cameras.size(); v++) {
        if (rt_view_adaptive_resolve(set, (int32_t)v, 0, nullptr, rgb8.data()) != RT_OK) return fail();
        if (rt_write_ppm(numbered(out_path, v, ".ppm").c_str(), p.width, p.height, rgb8.data()) != RT_OK) return fail();
        if (!map_path) continue;
        if (rt_view_adaptive_sample_map(set, (int32_t)v, spp.data()) != RT_OK) return fail();
        const std::vector<float> image(spp.begin(), spp.end());
        const std::string path = numbered(map_path, v, ".pfm");
        if (!write_pfm(path.c_str(), p.width, p.height, 1, image)) { fprintf(stderr, "error: cannot write sample map %s\n", path.c_str()); rt_view_adaptive_destroy(set); return 1; }
    }
    rt_view_adaptive_destroy(set);
    return 0;
}

int main(int argc, const char *argv[]) {
    const char *snap = getenv("RTAMD_SNAPSHOT");
    rt_host_scene *hs = nullptr;
    rt_render_params p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p;
    const char *out_path = nullptr;
    if (argc == 3) { // .txt scene: everything comes from the file
        int flavor = RT_INTEGRATOR_HW3;
        if (snap && strlen(snap) == 3 && snap[0] == 'h' && snap[1] == 'w' && snap[2] >= '1' && snap[2] <= '5') flavor = snap[2] - '0';
        if (rt_load_txt(argv[1], flavor, &hs, &p.width, &p.height, &p.samples, &p.ray_depth) != RT_OK) return die();
        if (flavor == RT_INTEGRATOR_HW1 || flavor == RT_INTEGRATOR_HW2) p.samples = 1;
        p.integrator = flavor;
        out_path = argv[2];
    } else if (argc >= 6) {
        int flavor = (snap && strcmp(snap, "hw6") == 0) ? RT_INTEGRATOR_HW6 : RT_INTEGRATOR_HW8;
        const bool hw7 = snap && strcmp(snap, "hw7") == 0; // hw7 = the hw8 scene representation rendered with hw7's material model
        if (rt_load_gltf(argv[1], flavor, &hs) != RT_OK) return die();
        p.width = (int32_t)strtol(argv[2], nullptr, 10);
        p.height = (int32_t)strtol(argv[3], nullptr, 10);
        p.samples = (int32_t)strtol(argv[4], nullptr, 10);
        p.integrator = hw7 ? RT_INTEGRATOR_HW7 : flavor;
        out_path = argv[5];
        if (argc > 6 && rt_host_scene_set_environment(hs, argv[6]) != RT_OK) return die();
    } else {
        fprintf(stderr, "usage: %s <scene.gltf> <width> <height> <samples> <out.ppm> [<envmap.png>]\n       %s <scene.txt> <out.ppm>\n", argv[0], argv[0]);
        return 2;
    }
    rt_scene_desc desc = *rt_host_scene_desc(hs);
    // RTAMD_FAST_BUILD=1: scene tree built on the GPU, frames follow the reference's estimator instead of its pixels (rtamd.h);
    // RTAMD_STREAMS=k: throughput mode with k random streams per pixel
    if (getenv("RTAMD_FAST_BUILD") && desc.normals) desc.build_flags |= RT_BUILD_DEVICE_BVH;
    if (const char *e = getenv("RTAMD_STREAMS")) { int v = atoi(e); if (v > 1) p.sample_streams = v; }
    std::vector<uint8_t> rgb8(rt_output_elems(&p));
    if (rgb8.empty()) { fprintf(stderr, "error: bad image size %dx%d\n", p.width, p.height); return 1; }
    rt_stats st;
    int n_dev = rt_device_count();
    if (const char *e = getenv("RTAMD_DEVICES")) { int v = atoi(e); if (v >= 1 && v < n_dev) n_dev = v; }
    int slice = getenv("RTAMD_SLICE") ? atoi(getenv("RTAMD_SLICE")) : 0;
    const char *checkpoint = getenv("RTAMD_CHECKPOINT");
    NoiseTarget noise;
    if (argc >= 6) {
        if (const char *e = getenv("RTAMD_TARGET_NOISE")) {
            char *end = nullptr;
            noise.target = strtod(e, &end);
            if (end == e || *end != 0 || !std::isfinite(noise.target) || !(noise.target > 0)) { fprintf(stderr, "error: RTAMD_TARGET_NOISE must be a positive finite number (got \"%s\")\n", e); return 1; }
        }
        if (const char *e = getenv("RTAMD_NOISE_MIN_BATCHES")) { noise.min_batches = atoi(e); if (noise.min_batches < 2) noise.min_batches = 2; }
        noise.map = getenv("RTAMD_NOISE_MAP");
    }
    Preview preview;
    if (const char *e = getenv("RTAMD_DENOISE")) {
        if (argc < 6 || p.integrator == RT_INTEGRATOR_HW6) fprintf(stderr, "note: RTAMD_DENOISE serves the glTF surface with hw8 / hw7 (guide images are made for those scenes): no preview is written\n");
        else if (p.sample_streams > 1) fprintf(stderr, "note: RTAMD_DENOISE previews a resumable render, which throughput mode (RTAMD_STREAMS) is not: no preview is written\n");
        else { preview.path = e; preview.albedo = getenv("RTAMD_DENOISE_ALBEDO") && atoi(getenv("RTAMD_DENOISE_ALBEDO")) != 0; }
    }
    const bool sliced = argc >= 6 && (getenv("RTAMD_SLICE") || checkpoint || noise.active() || preview.path);
    if (sliced && slice <= 0 && getenv("RTAMD_SLICE")) { fprintf(stderr, "error: RTAMD_SLICE must be a positive number of samples\n"); return 1; }
    if (noise.active() && !getenv("RTAMD_SLICE")) slice = p.samples / 16 > 1 ? p.samples / 16 : 1; // watching the noise implies slices
    std::vector<int> list; // RTAMD_DEVICE_LIST: the devices of rt_multi_create, as given
    if (const char *e = getenv("RTAMD_DEVICE_LIST")) {
        const int visible = rt_device_count();
        for (const char *c = e;;) {
            char *end = nullptr;
            const long v = strtol(c, &end, 10);
            if (end == c || c[0] == '-' || c[0] == '+' || c[0] == ' ' || v >= visible || list.size() >= 64 || (*end != ',' && *end != 0)) {
                fprintf(stderr, "error: RTAMD_DEVICE_LIST must be 1 to 64 HIP device indices below %d separated by commas, e.g. 0,1 (got \"%s\")\n", visible, e);
                return 1;
            }
            list.push_back((int)v);
            if (*end == 0) break;
            c = end + 1;
        }
        n_dev = (int)list.size();
    }
    const bool adaptive = argc >= 6 && getenv("RTAMD_ADAPTIVE") && atoi(getenv("RTAMD_ADAPTIVE")) != 0;
    if (adaptive) { // one GPU and hw8 only; what else stands in the way is the library's to say (rt_adaptive_create)
        const char *why = !(noise.target > 0) ? "it needs RTAMD_TARGET_NOISE=x, the noise at which a sub-tile stops"
                          : p.integrator != RT_INTEGRATOR_HW8 ? "it runs the hw8 integrator only (RTAMD_SNAPSHOT=hw8, the default)"
                          : (!list.empty() || n_dev > 1) ? "it runs on one GPU (RTAMD_DEVICES=1; no RTAMD_DEVICE_LIST)"
                          : checkpoint ? "an adaptive render has no checkpoint (RTAMD_CHECKPOINT)"
                          : preview.path ? "an adaptive render has no denoised preview (RTAMD_DENOISE)" : nullptr;
        if (why) { fprintf(stderr, "error: RTAMD_ADAPTIVE: %s\n", why); return 1; }
    }
    std::vector<rt_camera> cameras; // RTAMD_CAMERAS: one GPU and hw8 only; what else stands in the way is the library's to say (rt_views_create)
    if (const char *path = argc >= 6 ? rtamd::env_str("RTAMD_CAMERAS") : nullptr) {
        const char *why = p.integrator != RT_INTEGRATOR_HW8 ? "it runs the hw8 integrator only (RTAMD_SNAPSHOT=hw8, the default)"
                          : (!list.empty() || n_dev > 1) ? "it runs on one GPU (RTAMD_DEVICES=1; no RTAMD_DEVICE_LIST)"
                          : (checkpoint || preview.path || (adaptive ? noise.map != nullptr : noise.active())) ? // with RTAMD_ADAPTIVE the target is the sub-tiles'
"a view set has no checkpoint, noise monitor or denoised preview (RTAMD_CHECKPOINT, RTAMD_TARGET_NOISE, RTAMD_NOISE_MAP, RTAMD_DENOISE)"
                          : p.sample_streams > 1 ? "a view set renders in replay mode (no RTAMD_STREAMS)" : nullptr;
        if (why) { fprintf(stderr, "error: RTAMD_CAMERAS: %s\n", why); return 1; }
        if (!read_cameras(path, cameras)) return 1;
    }
    rt_multi *multi = nullptr; // all devices, or ...
    rt_scene *scene = nullptr; // ... one
    if ((!list.empty() || n_dev > 1) && p.integrator != RT_INTEGRATOR_HW1) {
        if (rt_multi_create(&desc, list.empty() ? nullptr : list.data(), n_dev, &multi) != RT_OK) return die();
    } else if (rt_scene_create(&desc, &scene) != RT_OK) return die();
    if (const char *prefix = argc >= 6 ? getenv("RTAMD_GUIDES") : nullptr) { // before the frame, which they do not touch
        rt_scene *own = nullptr; // a guide pass runs on one device: with several, on a scene of its own on the current one
        if (!scene && rt_scene_create(&desc, &own) != RT_OK) return die();
        const int rc = write_guides(scene ? scene : own, p, prefix);
        rt_scene_destroy(own);
        if (rc) return rc;
    }
    if (!cameras.empty()) {
        const int rc = adaptive ? render_view_adaptive(scene, p, slice, noise, cameras, out_path, rgb8) : render_views(scene, p, slice, cameras, out_path, rgb8);
        rt_scene_destroy(scene);
        rt_host_scene_free(hs);
        if (rc == 0) fprintf(stderr, "FINISH\n");
        return rc;
    }
    if (adaptive) {
        const int rc = render_adaptive(scene, p, slice, noise, out_path, rgb8);
        rt_scene_destroy(scene);
        rt_host_scene_free(hs);
        if (rc == 0) fprintf(stderr, "FINISH\n");
        return rc;
    }
    if (sliced) {
        Progress acc;
        if ((multi ? rt_multi_accum_create(multi, &p, &acc.all) : rt_accum_create(scene, &p, &acc.one)) != RT_OK) return die();
        if (preview.path && multi && rt_scene_create(&desc, &preview.scene) != RT_OK) return die();
        const int rc = render_in_slices(acc, p, slice, checkpoint, out_path, rgb8, noise, preview);
        acc.destroy(); // before its rt_multi or its scene
        rt_scene_destroy(preview.scene);
        rt_multi_destroy(multi);
        rt_scene_destroy(scene);
        rt_host_scene_free(hs);
        if (rc == 0) fprintf(stderr, "FINISH\n");
        return rc < 0 ? 0 : rc; // < 0: stopped by RTAMD_SLICE_LIMIT, the checkpoint and the picture so far are written
    }
    if (multi) {
        if (rt_multi_render(multi, &p, nullptr, rgb8.data(), &st) != RT_OK) return die();
        fprintf(stderr, "render: %d GPUs, slowest %.3f ms, %.2f Msamples/s over the whole call\n", n_dev, st.kernel_ms, st.samples / (st.total_ms * 1e3));
        rt_multi_destroy(multi);
    } else {
        if (rt_render(scene, &p, nullptr, rgb8.data(), &st) != RT_OK) return die();
        fprintf(stderr, "render: %.3f ms on the GPU, %.2f Msamples/s\n", st.kernel_ms, st.samples / (st.kernel_ms * 1e3));
        if ((p.integrator == RT_INTEGRATOR_HW8 || p.integrator == RT_INTEGRATOR_HW7 || p.integrator == RT_INTEGRATOR_HW6) && !st.reference_exact)
            fprintf(stderr, "note: this render kept the answers of the walkers' padded boxes (no exactness gate on this path: see rt_stats.reference_exact in rtamd.h); about one pixel in 1e5 may differ from the reference's\n");
        rt_scene_destroy(scene);
    }
    if (rt_write_ppm(out_path, p.width, p.height, rgb8.data()) != RT_OK) return die();
    rt_host_scene_free(hs);
    fprintf(stderr, "FINISH\n");
    return 0;
}
