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
#include "../../../include/rtamd.h"
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

// The frame in slices: the picture after every slice is the frame of that many samples, the last one the frame of the plain run.
// `p` are the params of the unsharded frame, whose rt_accum_state_bytes is the size of the checkpoint on any number of devices.
static int render_in_slices(Progress &acc, const rt_render_params &p, int slice, const char *checkpoint, const char *out_path, std::vector<uint8_t> &rgb8) {
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
    const int limit = getenv("RTAMD_SLICE_LIMIT") ? atoi(getenv("RTAMD_SLICE_LIMIT")) : 0;
    const std::string tmp_ppm = std::string(out_path) + ".part";
    double kernel_ms = 0;
    uint64_t samples = 0;
    uint32_t exact = 1;
    for (int k = 0;; k++) {
        const int done = acc.samples();
        if (k > 0 || done == p.samples) { // the picture so far (a checkpoint that already holds the frame just resolves)
            if (acc.resolve(rgb8.data()) != RT_OK) return die();
            if (rt_write_ppm(tmp_ppm.c_str(), p.width, p.height, rgb8.data()) != RT_OK) return die();
            if (rename(tmp_ppm.c_str(), out_path) != 0) { fprintf(stderr, "error: cannot rename %s to %s\n", tmp_ppm.c_str(), out_path); return 1; }
        }
        if (done == p.samples) break;
        if (limit > 0 && k >= limit) {
            fprintf(stderr, "STOPPED after %d slices at %d of %d samples\n", k, done, p.samples);
            acc.destroy();
            return -1;
        }
        const int n = slice > 0 && slice < p.samples - done ? slice : p.samples - done;
        rt_stats st;
        if (acc.render(n, &st) != RT_OK) return die();
        kernel_ms += st.kernel_ms; samples += st.samples; exact &= st.reference_exact;
        fprintf(stderr, "slice %d: %d samples (%d of %d), %.3f ms on the GPU\n", k + 1, n, done + n, p.samples, st.kernel_ms);
        if (checkpoint) {
            if (acc.save(blob.data(), blob.size()) != RT_OK) return die();
            if (!write_file_atomically(checkpoint, blob.data(), blob.size())) { fprintf(stderr, "error: cannot write checkpoint %s\n", checkpoint); return 1; }
        }
    }
    if (samples) fprintf(stderr, "render: %.3f ms on the GPU, %.2f Msamples/s\n", kernel_ms, samples / (kernel_ms * 1e3));
    if (samples && !exact)
        fprintf(stderr, "note: this render kept the answers of the walkers' padded boxes (no exactness gate on this path: see rt_stats.reference_exact in rtamd.h); about one pixel in 1e5 may differ from the reference's\n");
    acc.destroy();
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
    const int slice = getenv("RTAMD_SLICE") ? atoi(getenv("RTAMD_SLICE")) : 0;
    const char *checkpoint = getenv("RTAMD_CHECKPOINT");
    const bool sliced = argc >= 6 && (getenv("RTAMD_SLICE") || checkpoint);
    if (sliced && slice <= 0 && getenv("RTAMD_SLICE")) { fprintf(stderr, "error: RTAMD_SLICE must be a positive number of samples\n"); return 1; }
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
    if ((!list.empty() || n_dev > 1) && p.integrator != RT_INTEGRATOR_HW1) {
        rt_multi *multi = nullptr;
        if (rt_multi_create(&desc, list.empty() ? nullptr : list.data(), n_dev, &multi) != RT_OK) return die();
        if (sliced) {
            Progress acc;
            if (rt_multi_accum_create(multi, &p, &acc.all) != RT_OK) return die();
            const int rc = render_in_slices(acc, p, slice, checkpoint, out_path, rgb8);
            acc.destroy(); // before its rt_multi
            rt_multi_destroy(multi);
            rt_host_scene_free(hs);
            if (rc == 0) fprintf(stderr, "FINISH\n");
            return rc < 0 ? 0 : rc; // < 0: stopped by RTAMD_SLICE_LIMIT, the checkpoint and the picture so far are written
        }
        if (rt_multi_render(multi, &p, nullptr, rgb8.data(), &st) != RT_OK) return die();
        fprintf(stderr, "render: %d GPUs, slowest %.3f ms, %.2f Msamples/s over the whole call\n", n_dev, st.kernel_ms, st.samples / (st.total_ms * 1e3));
        rt_multi_destroy(multi);
    } else {
        rt_scene *scene = nullptr;
        if (rt_scene_create(&desc, &scene) != RT_OK) return die();
        if (sliced) {
            Progress acc;
            if (rt_accum_create(scene, &p, &acc.one) != RT_OK) return die();
            const int rc = render_in_slices(acc, p, slice, checkpoint, out_path, rgb8);
            acc.destroy(); // before its scene
            rt_scene_destroy(scene);
            rt_host_scene_free(hs);
            if (rc == 0) fprintf(stderr, "FINISH\n");
            return rc < 0 ? 0 : rc; // < 0: stopped by RTAMD_SLICE_LIMIT, the checkpoint and the picture so far are written
        }
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
