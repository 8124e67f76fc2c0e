// Sanitizer driver: the product's host library sources (scene / kd / BVH build, OBJ + MTL,
// PNG / HDR decoding, rgb2spec, C API) and the oracle built together with AddressSanitizer +
// UndefinedBehaviorSanitizer (`make sanitize`; CPU only, no HIP).  It exercises
//   1. the Cornell box, path tracing and BDPT tiles through the oracle;
//   2. a scene with every texture kind (PNG image, Radiance HDR environment, checkerboard,
//      marble, Mandelbrot, bump map, textured light), both integrators;
//   3. the decoders on hostile input: truncated and bit-flipped PNG / HDR files and mangled
//      OBJ / MTL text must fail cleanly (or load) without any sanitizer report;
//   4. the tile-task generator and instance transforms;
//   5. the render schedulers' plan and task groups (csrc/common/sched_plan.h) against recorded plans.
// Any ASan / UBSan finding aborts the process (halt_on_error), which the test treats as failure.
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/lumo_host.h"
#include "../../lumo_amd/csrc/common/sched_plan.h"
#include "../../oracle/oracle.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void put32(std::vector<uint8_t>& v, uint32_t x) {
    for (int s = 24; s >= 0; s -= 8) v.push_back((uint8_t)(x >> s));
}
void chunk(std::vector<uint8_t>& out, const char* tag, const std::vector<uint8_t>& data) {
    put32(out, (uint32_t)data.size());
    std::vector<uint8_t> td(tag, tag + 4);
    td.insert(td.end(), data.begin(), data.end());
    out.insert(out.end(), td.begin(), td.end());
    put32(out, (uint32_t)crc32(0, td.data(), (uInt)td.size()));
}
// An 8-bit PNG of colour type ct (2 RGB, 6 RGBA, 0 grey, 3 palette) with random pixels; rows
// use filter r % 5 applied to raw bytes of zero-predicted content (valid for every filter type).
std::vector<uint8_t> png(int w, int h, int ct) {
    const int ch = ct == 2 ? 3 : ct == 6 ? 4 : 1;
    std::vector<uint8_t> raw;
    for (int y = 0; y < h; ++y) {
        raw.push_back(0);
        for (int x = 0; x < w * ch; ++x) raw.push_back((uint8_t)(ct == 3 ? rnd() % 4 : rnd()));
    }
    uLongf n = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(n);
    compress2(z.data(), &n, raw.data(), (uLong)raw.size(), 6);
    z.resize(n);
    std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::vector<uint8_t> ihdr;
    put32(ihdr, (uint32_t)w);
    put32(ihdr, (uint32_t)h);
    ihdr.insert(ihdr.end(), {8, (uint8_t)ct, 0, 0, 0});
    chunk(out, "IHDR", ihdr);
    if (ct == 3) {
        std::vector<uint8_t> pal;
        for (int i = 0; i < 12; ++i) pal.push_back((uint8_t)rnd());
        chunk(out, "PLTE", pal);
    }
    chunk(out, "IDAT", z);
    chunk(out, "IEND", {});
    return out;
}
std::vector<uint8_t> hdr(int w, int h) {
    std::string head = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y " + std::to_string(h) + " +X " + std::to_string(w) + "\n";
    std::vector<uint8_t> out(head.begin(), head.end());
    for (int i = 0; i < w * h; ++i) {
        for (int k = 0; k < 3; ++k) out.push_back((uint8_t)rnd());
        out.push_back((uint8_t)(124 + rnd() % 8));
    }
    return out;
}

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); \
            std::exit(2);                                                \
        }                                                                \
    } while (0)

// Render `res` x `res` at `spp` with the oracle (both integrators) and check the output is finite.
void render(void* scene, const lumo_camera_params& cp, int res, int spp) {
    lumo_scene_desc d;
    CHECK(lumo_scene_get_desc(scene, &d) == 0);
    lumo_camera_params p = cp;
    p.width = p.height = res;
    lumo_camera_desc cam;
    CHECK(lumo_camera_build(&p, &cam) == 0);
    const int64_t n = lumo_make_tasks(res, res, (uint64_t)spp, 77, nullptr, 0);
    CHECK(n > 0);
    std::vector<lumo_tile_task> tasks((size_t)n);
    CHECK(lumo_make_tasks(res, res, (uint64_t)spp, 77, tasks.data(), n) == n);
    for (int integ : {LUMO_INTEGRATOR_PATH_TRACE, LUMO_INTEGRATOR_BDPT}) {
        oracle_set_integrator(integ);
        std::vector<std::vector<double>> bufs((size_t)n);
        std::vector<std::vector<lumo_splat>> sp((size_t)n);
        std::vector<lumo_tile_result> res_((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const lumo_tile_task& t = tasks[(size_t)i];
            const uint64_t px = (t.px_max[0] - t.px_min[0]) * (t.px_max[1] - t.px_min[1]);
            bufs[(size_t)i].assign(4 * px, 0.0);
            sp[(size_t)i].resize(64 * px * t.samples);
            res_[(size_t)i] = lumo_tile_result{};
            res_[(size_t)i].rgb_w = bufs[(size_t)i].data();
            if (integ == LUMO_INTEGRATOR_BDPT) {
                res_[(size_t)i].splats = sp[(size_t)i].data();
                res_[(size_t)i].splat_cap = sp[(size_t)i].size();
            }
        }
        oracle_counters c{};
        CHECK(oracle_render_tiles(&d, &cam, tasks.data(), (size_t)n, 0, 2, res_.data(), &c) == 0);
        double sum = 0.0;
        for (const auto& b : bufs)
            for (double v : b) {
                CHECK(v == v);
                sum += v;
            }
        CHECK(sum > 0.0);
    }
    oracle_set_integrator(LUMO_INTEGRATOR_PATH_TRACE);
}

void cornell() {
    void* b = lumo_builder_cornell_box();
    void* s = lumo_builder_build(b);
    CHECK(s);
    lumo_camera_params cp;
    lumo_camera_params_cornell_box(&cp);
    render(s, cp, 24, 4);
    lumo_scene_free(s);
    lumo_builder_free(b);
}

void textured() {
    void* b = lumo_builder_new();
    const lumo_spectrum white = lumo_spectrum_from_rgb(0.8, 0.8, 0.8);
    const std::vector<uint8_t> img = png(7, 5, 2), pal = png(4, 4, 3), bump = png(5, 3, 2), lamp = png(3, 3, 6);
    const std::vector<uint8_t> env = hdr(8, 4);
    const int t_img = lumo_builder_texture_image(b, (const char*)img.data(), img.size());
    const int t_pal = lumo_builder_texture_image(b, (const char*)pal.data(), pal.size());
    const int t_marble = lumo_builder_texture_marble(b, 1234, white);
    const int t_man = lumo_builder_texture_mandelbrot(b);
    const int t_chk = lumo_builder_texture_checkerboard(b, t_marble, t_man, 5.0);
    const int t_lamp = lumo_builder_texture_image(b, (const char*)lamp.data(), lamp.size());
    const int t_env = lumo_builder_texture_hdr(b, (const char*)env.data(), env.size());
    const int nm = lumo_builder_normal_map(b, (const char*)bump.data(), bump.size());
    CHECK(t_img >= 0 && t_pal >= 0 && t_chk >= 0 && t_lamp >= 0 && t_env >= 0 && nm >= 0);
    const int left = lumo_builder_material_textured(b, lumo_builder_material_diffuse(b, white), t_chk, -1, -1, -1);
    const int right = lumo_builder_material_textured(b, lumo_builder_material_diffuse(b, white), t_img, -1, -1, -1);
    CHECK(lumo_builder_empty_box(b, white, left, right) == 0);
    const int bumpy = lumo_builder_material_textured(
        b, lumo_builder_material_microfacet(b, 0.4, 1.5, 0.0, 0, 0, white, white, lumo_spectrum_from_rgb(0, 0, 0)),
        t_pal, -1, -1, nm);
    const int metal = lumo_builder_material_textured(b, lumo_builder_material_metal(b, white, 0.3, 1.5, 3.0), -1, t_img,
                                                     -1, -1);
    const int glass = lumo_builder_material_textured(b, lumo_builder_material_transparent(b, white, 0.2, 1.5), -1, -1,
                                                     t_chk, -1);
    const char* cube =
        "v -0.2 -0.6 -1.2\nv 0.2 -0.6 -1.2\nv 0.2 -0.2 -1.2\nv -0.2 -0.2 -1.2\nv -0.2 -0.6 -1.6\nv 0.2 -0.6 -1.6\n"
        "v 0.2 -0.2 -1.6\nv -0.2 -0.2 -1.6\nvt 0 0\nvt 2 0\nvt 2 2\nvt 0 2\n"
        "f 1/1 2/2 3/3 4/4\nf 5/1 8/2 7/3 6/4\nf 4/1 3/2 7/3 8/4\nf 1/1 5/2 6/3 2/4\nf 2/1 6/2 7/3 3/4\nf 1/1 4/2 8/3 5/4\n";
    for (int m : {bumpy, metal, glass}) {
        const int64_t idx = lumo_builder_add_obj_mesh(b, cube, std::strlen(cube), m);
        CHECK(idx >= 0);
        CHECK(lumo_builder_instance_op(b, 0, idx, 0, 0.45 * (m - metal), 0.0, 0.1 * (m - metal)) == 0);
    }
    CHECK(lumo_builder_add_sphere(b, 0.2, lumo_builder_material_textured(b, lumo_builder_material_diffuse(b, white),
                                                                          t_marble, -1, -1, -1), 0) == 0);
    CHECK(lumo_builder_instance_op(b, 0, lumo_builder_count(b, 0) - 1, 0, 0.0, 0.3, -1.5) == 0);
    const int lm = lumo_builder_material_textured(b, lumo_builder_material_light(b, white, LUMO_DENSE_D65, 4.0, 0),
                                                  t_lamp, -1, -1, -1);
    const double a[3] = {-0.25, 0.79, -1.4}, bb[3] = {0.25, 0.79, -1.4}, c[3] = {0.25, 0.79, -0.9};
    CHECK(lumo_builder_add_rectangle(b, a, bb, c, lm, 1) == 0);
    CHECK(lumo_builder_set_environment_texture(b, t_env, 0.5) == 0);
    void* s = lumo_builder_build(b);
    CHECK(s);
    lumo_camera_params cp;
    lumo_camera_params_default(&cp);
    render(s, cp, 16, 4);
    lumo_scene_free(s);
    lumo_builder_free(b);
}

// Decoders on hostile input: must return an error or a valid texture, never fault.
void hostile() {
    const std::vector<std::vector<uint8_t>> seeds = {png(6, 4, 2), png(5, 5, 6), png(4, 3, 0), png(6, 2, 3), hdr(4, 3)};
    int ok = 0, bad = 0;
    for (int it = 0; it < 600; ++it) {
        std::vector<uint8_t> f = seeds[(size_t)(it % seeds.size())];
        const int mode = it % 3;
        if (mode == 0) {
            f.resize(rnd() % f.size());
        } else {
            const int flips = 1 + (int)(rnd() % 8);
            for (int k = 0; k < flips; ++k) f[rnd() % f.size()] ^= (uint8_t)(1u << (rnd() % 8));
        }
        void* b = lumo_builder_new();
        const bool is_hdr = (it % seeds.size()) == seeds.size() - 1;
        const int t = is_hdr ? lumo_builder_texture_hdr(b, (const char*)f.data(), f.size())
                             : lumo_builder_texture_image(b, (const char*)f.data(), f.size());
        const int n = is_hdr ? -1 : lumo_builder_normal_map(b, (const char*)f.data(), f.size());
        (t >= 0 ? ok : bad)++;
        (void)n;
        lumo_builder_free(b);
    }
    CHECK(ok > 0 && bad > 0);
    // HDR headers whose sizes overflow the texel count (the count wraps to 0, so the data-size
    // check alone would pass an empty body) or exceed the int32 texel indexing
    for (const char* hd : {"#?RADIANCE\n-Y 4 +X 4611686018427387904\n", "#?RADIANCE\n-Y 4611686018427387904 +X 4\n",
                           "#?RADIANCE\n-Y 65536 +X 65536\n", "#?RADIANCE\n-Y 1 +X 2147483648\n"}) {
        void* b = lumo_builder_new();
        CHECK(lumo_builder_texture_hdr(b, hd, std::strlen(hd)) < 0);
        lumo_builder_free(b);
    }
    // mangled OBJ / MTL text
    const std::string obj = "mtllib a.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvn 0 0 1\n"
                            "usemtl m\nf 1/1/1 2/2/1 3/3/1\nf 2 4 3\nusemtl l\nf -1 -2 -3\n";
    const std::string mtl = "newmtl m\nKd 0.5 0.5 0.5\nNs 10\nillum 5\nmap_Kd t.png\nnewmtl l\nKe 1 1 1\n";
    const std::vector<uint8_t> tp = png(3, 3, 2);
    for (int it = 0; it < 400; ++it) {
        std::string o = obj, m = mtl;
        std::string& x = (it % 2) ? o : m;
        const int edits = 1 + (int)(rnd() % 6);
        for (int k = 0; k < edits; ++k) {
            const size_t pos = rnd() % x.size();
            switch (rnd() % 4) {
                case 0: x.erase(pos, 1 + rnd() % 4); break;
                case 1: x.insert(pos, 1, "-/ 0123456789\nfvtn."[rnd() % 19]); break;
                case 2: x[pos] = (char)(rnd() % 128); break;
                default: x.insert(pos, "f 99 -99 0/0/0\n"); break;
            }
            if (x.empty()) x = "v";
        }
        void* b = lumo_builder_new();
        lumo_builder_add_file(b, "t.png", (const char*)tp.data(), tp.size());
        if (lumo_builder_load_obj_scene(b, o.data(), o.size(), m.data(), m.size()) == 0) {
            void* s = lumo_builder_build(b);
            if (s) lumo_scene_free(s);
        }
        lumo_builder_free(b);
    }
}

void tasks() {
    for (int it = 0; it < 50; ++it) {
        const int64_t w = 1 + (int64_t)(rnd() % 70), h = 1 + (int64_t)(rnd() % 70);
        const uint64_t spp = 1 + rnd() % 600;
        const int64_t n = lumo_make_tasks(w, h, spp, rnd(), nullptr, 0);
        std::vector<lumo_tile_task> t((size_t)n);
        CHECK(lumo_make_tasks(w, h, spp, 3, t.data(), n) == n);
    }
}

// oracle_trace on Cornell in the wide and the two brute-force modes (oracle_set_accel 1 / 2 / 3):
// axis-parallel rays with both signs of zero and rays aimed at a corner of the scene; the modes
// agree on t.
void brute() {
    void* b = lumo_builder_cornell_box();
    void* s = lumo_builder_build(b);
    CHECK(s);
    lumo_scene_desc d;
    CHECK(lumo_scene_get_desc(s, &d) == 0);
    const size_t n = 600;
    std::vector<double> o(3 * n), dir(3 * n), t[3];
    std::vector<int32_t> kind(n), obj(n), prim(n), light(n, 0);
    for (size_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) o[3 * i + a] = 1.0 + (double)(rnd() % 5400) / 10.0;
        if (i % 2) {
            for (int a = 0; a < 3; ++a) dir[3 * i + a] = (rnd() & 1) ? 0.0 : -0.0;
            dir[3 * i + rnd() % 3] = (rnd() & 1) ? 1.0 : -1.0;
        } else {
            double len = 0.0;
            for (int a = 0; a < 3; ++a) {
                dir[3 * i + a] = d.vertices[a] - o[3 * i + a];
                len += dir[3 * i + a] * dir[3 * i + a];
            }
            for (int a = 0; a < 3; ++a) dir[3 * i + a] /= std::sqrt(len);
        }
    }
    const lumo_ray_soa rays{o.data(), dir.data(), nullptr, light.data()};
    for (int any = 0; any < 2; ++any) {
        for (int m = 0; m < 3; ++m) {
            t[m].assign(n, 0.0);
            lumo_hit_soa hits{t[m].data(), kind.data(), obj.data(), prim.data()};
            oracle_counters c{};
            oracle_set_accel(m + 1);
            CHECK(oracle_trace(&d, &rays, n, &hits, any, &c) == 0);
        }
        oracle_set_accel(0);
        for (size_t i = 0; i < n; ++i) CHECK(t[0][i] == t[1][i] && t[1][i] == t[2][i]);
    }
    lumo_scene_free(s);
    lumo_builder_free(b);
}

// The schedule plan (sched_plan.h plan_schedule) against the plans the device code chose before the
// plan was one function.  "test": the tuple a GPU test asserts through lumo_last_schedule; the other
// fields of those rows, and the rows without a test, were evaluated by hand from the expressions of
// lumo_amd/csrc/device/kernels.hip at commit 655ab47 (cited by line).
void plans() {
    using lumo::dev::SchedIn;
    using lumo::dev::SchedPlan;
    const size_t GiB = (size_t)1 << 30, plenty = 256 * GiB;
    // the default options (ctx.h Opts), a staged n_shadow == 1 scene that fits (Cornell), no memory figures
    SchedIn c1{};
    c1.fused = -1, c1.lds = 1, c1.pipeline = 3, c1.heads = 0, c1.merge = 0, c1.tail_bounces = -1;
    c1.split_pipe = 4, c1.split_groups = 2, c1.bdpt_groups = 2;
    c1.n_shadow = 1, c1.staged = true, c1.fused_fits = true, c1.max_merge = 8, c1.rr_depth = 5;  // state.h
    c1.N = 1536 * 1536, c1.n_tasks = 96 * 96, c1.max_samples = 8;
    // C3: n_shadow == 11, too large to stage; 7 000 B per slot and set (a figure of the right size), plenty free
    SchedIn c3 = c1;
    c3.n_shadow = 11, c3.staged = false, c3.fused_fits = false;
    c3.N = 1920 * 1080, c3.n_tasks = 8160, c3.max_samples = 2;
    c3.set_bytes_slot = 7000, c3.set_bytes_fixed = 1 << 16, c3.free_hbm = plenty, c3.held = 0, c3.hbm_known = true;
    const size_t c3_set = c3.set_bytes_fixed + c3.set_bytes_slot * (size_t)c3.N;
    // the 64x48 mid-size scenes of tests/test_gpu_scale.py: 12 tasks, 9 spp
    SchedIn mid = c3;
    mid.N = 64 * 48, mid.n_tasks = 12, mid.max_samples = 9;
    struct Case {
        const char* name;
        SchedIn in;
        SchedPlan want;  // schedule, fused, M, K, G, head streams, head bounces, tail bounces
    };
    std::vector<Case> cases;
    auto add = [&](const char* name, SchedIn in, SchedPlan want) { cases.push_back({name, in, want}); };
    // test_gpu_parity.py test_headline_schedule_matches_oracle: (1, 3 streams, 6 heads, M 1, tail 2)
    add("headline", c1, {1, true, 1, 1, 1, 3, 6, 2});
    {   // ... its second render, pipeline 0: schedule 0 (2037, 2040: no pipeline, no split)
        SchedIn in = c1;
        in.pipeline = 0;
        add("headline, pipeline 0", in, {0, true, 1, 1, 1, 0, 0, 0});
    }
    {   // test_share_schedule_matches_sequential_and_oracle: (1, 3, M 8); heads min(5, RR_DEPTH) (1078-1079),
        // tail bounces 0 for merged units (1083)
        SchedIn in = c1;
        in.N = 131072, in.n_tasks = 512, in.max_samples = 24;
        add("C1 share", in, {1, true, 8, 1, 1, 3, 5, 0});
        in.max_samples = 3;  // M <= max_samples (2049)
        add("C1 share, 3 spp", in, {1, true, 3, 1, 1, 3, 5, 0});
        in.heads = 7, in.tail_bounces = 1, in.pipeline = 1;  // test_gpu_options.py: heads capped for merged units
        add("C1 share, options", in, {1, true, 3, 1, 1, 1, 5, 1});
        in.merge = 1, in.pipeline = 5;  // one-pass units keep the requested heads; at most 3 head streams (1051)
        add("C1 share, merge 1", in, {1, true, 1, 1, 1, 3, 7, 1});
    }
    {   // N x M > 2^30: M falls to 1 (2050); N >= 2^21: 6 heads
        SchedIn in = c1;
        in.N = 1 << 28, in.merge = 8;
        add("huge pass", in, {1, true, 1, 1, 1, 3, 6, 2});
    }
    {   // a dump of a fused scene runs the fused pipeline (2037 has no dump term; the smoke run's path dump):
        // 32x32, 4 spp: M = min(8, 2048, 4) (2043-2049)
        SchedIn in = c1;
        in.dump = true, in.N = 1024, in.n_tasks = 1, in.max_samples = 4;
        add("fused dump", in, {1, true, 4, 1, 1, 3, 5, 0});
    }
    {   // fused by option and by fit (2033-2036)
        SchedIn in = c1;
        in.fused_fits = false;
        in.hbm_known = true, in.free_hbm = plenty, in.set_bytes_slot = 700;
        add("does not fit", in, {2, false, 1, 4, 2, 0, 0, 0});
        in.fused = 1;
        add("fused forced", in, {1, true, 1, 1, 1, 3, 6, 2});
        in.fused = 0, in.fused_fits = true;
        add("fused off", in, {2, false, 1, 4, 2, 0, 0, 0});
        in.fused = -1, in.lds = 0;
        add("lds off", in, {2, false, 1, 4, 2, 0, 0, 0});
    }
    // test_gpu_scale.py test_c3_bench_schedule_full_frame: (2, K 4, G 2, fused 0); M 1 (2047)
    add("C3 frame", c3, {2, false, 1, 4, 2, 0, 0, 0});
    {   // a dump of the split bounces: sequential (2040)
        SchedIn in = c3;
        in.dump = true, in.N = 1024, in.n_tasks = 1, in.max_samples = 4;
        add("split dump", in, {0, false, 1, 1, 1, 0, 0, 0});
    }
    {   // split_pipe 1: sequential, whatever merge asks (test_c3_share_merged_passes' second render; 2040)
        SchedIn in = c3;
        in.split_pipe = 1, in.merge = 8;
        add("split_pipe 1", in, {0, false, 1, 1, 1, 0, 0, 0});
    }
    {   // free memory (2232-2237): K - 1 extra sets and the 8 GiB margin must fit in free + held
        SchedIn in = c3;
        in.free_hbm = 9 * GiB;
        add("low memory", in, {0, false, 1, 1, 1, 0, 0, 0});
        in.free_hbm = 8 * GiB + c3_set;
        add("one extra set fits", in, {2, false, 1, 2, 2, 0, 0, 0});
        in.free_hbm = 8 * GiB + 2 * c3_set - 1;
        add("two extra sets do not", in, {2, false, 1, 2, 2, 0, 0, 0});
        in.held = 1;
        add("... with the byte held", in, {2, false, 1, 3, 2, 0, 0, 0});
        in.free_hbm = 0, in.held = 8 * GiB + 3 * c3_set;
        add("sets already held", in, {2, false, 1, 4, 2, 0, 0, 0});
        in.hbm_known = false;  // the query failed (2235)
        add("memory unknown", in, {0, false, 1, 1, 1, 0, 0, 0});
    }
    {   // test_c3_share_merged_passes: (2, K 4, G 2, M 8)
        SchedIn in = c3;
        in.N = 261120, in.n_tasks = 1020, in.max_samples = 16, in.merge = 8;
        add("C3 share, merge 8", in, {2, false, 8, 4, 2, 0, 0, 0});
    }
    // test_split_pipeline_passes_in_flight (k, groups): (2, k, min(groups, k)); k = 1: schedule 0
    for (int k = 1; k <= 4; ++k)
        for (int groups : {1, 2, 3, 4}) {
            SchedIn in = mid;
            in.split_pipe = k, in.split_groups = groups, in.merge = 1;
            add("units in flight", in, k == 1 ? SchedPlan{0, false, 1, 1, 1, 0, 0, 0}
                                              : SchedPlan{2, false, 1, k, std::min(groups, k), 0, 0, 0});
        }
    {   // test_split_merged_passes (merge, k, groups): (2, k, min(groups, k), M merge); a forced merge with
        // the split schedule
        const int rows[5][3] = {{8, 4, 2}, {2, 4, 2}, {3, 3, 1}, {8, 4, 4}, {4, 2, 2}};
        for (const auto& r : rows) {
            SchedIn in = mid;
            in.merge = r[0], in.split_pipe = r[1], in.split_groups = r[2];
            add("split, merged", in, {2, false, r[0], r[1], std::min(r[2], r[1]), 0, 0, 0});
        }
        SchedIn in = mid;  // fewer units than sets: 9 passes in units of 8, one group: 2 units (2233-2236)
        in.merge = 8, in.split_groups = 1;
        add("split, two units", in, {2, false, 8, 2, 1, 0, 0, 0});
        in.max_samples = 1, in.n_tasks = 1;  // one unit: nothing to pipeline (2039-2040)
        add("split, one unit", in, {0, false, 1, 1, 1, 0, 0, 0});
    }
    {   // BDPT (2255-2259, 1637): test_gpu_bdpt.py (3, groups) for several tasks, (0, 1) for one group
        SchedIn in = c1;
        in.bdpt = true, in.N = 1024, in.n_tasks = 1, in.max_samples = 4;
        add("BDPT, one task", in, {0, true, 1, 1, 1, 0, 0, 0});
        in.N = 64 * 48, in.n_tasks = 12;
        add("BDPT, 12 tasks", in, {3, true, 1, 2, 2, 0, 0, 0});
        in.bdpt_groups = 9;
        add("BDPT, 9 groups asked", in, {3, true, 1, 4, 4, 0, 0, 0});
        in.n_tasks = 3;
        add("BDPT, 3 tasks", in, {3, true, 1, 3, 3, 0, 0, 0});
        in.bdpt_groups = 1;
        add("BDPT, groups 1", in, {0, true, 1, 1, 1, 0, 0, 0});
        in.bdpt_groups = 0;
        add("BDPT, groups 0", in, {0, true, 1, 1, 1, 0, 0, 0});
        in.bdpt_groups = 2, in.n_tasks = 1, in.dump = true;
        add("BDPT dump", in, {0, true, 1, 1, 1, 0, 0, 0});
        in = c3, in.bdpt = true;
        add("BDPT, C3", in, {3, false, 1, 2, 2, 0, 0, 0});
    }
    for (const Case& k : cases) {
        const SchedPlan p = lumo::dev::plan_schedule(k.in);
        const SchedPlan& w = k.want;
        if (p.schedule != w.schedule || p.fused != w.fused || p.M != w.M || p.K != w.K || p.G != w.G ||
            p.head_streams != w.head_streams || p.head_bounces != w.head_bounces || p.tail_bounces != w.tail_bounces) {
            std::fprintf(stderr, "plan \"%s\": got (%d, %d, M %d, K %d, G %d, %d, %d, %d)\n", k.name, p.schedule, (int)p.fused,
                         p.M, p.K, p.G, p.head_streams, p.head_bounces, p.tail_bounces);
            std::exit(2);
        }
    }
}

// task_groups (sched_plan.h) on 1, 2, 3 and 40 tasks of unequal size, every G <= min(4, tasks): the
// ranges are consecutive, cover the tasks, hold a task each, and are the ones the loop of
// kernels.hip:1319-1326 at commit 655ab47 yields (run on these sizes; the second 3-task case by hand).
void groups() {
    struct Case {
        std::vector<int> sizes;
        int G;
        std::vector<std::pair<int, int>> want;
    };
    std::vector<int> forty;
    for (int i = 0; i < 40; ++i) forty.push_back(1 + (i * 7) % 11);
    const std::vector<Case> cases = {
        {{5}, 1, {{0, 1}}},
        {{3, 10}, 1, {{0, 2}}},
        {{3, 10}, 2, {{0, 1}, {1, 2}}},
        {{7, 1, 4}, 1, {{0, 3}}},
        {{7, 1, 4}, 2, {{0, 1}, {1, 3}}},
        {{7, 1, 4}, 3, {{0, 1}, {1, 2}, {2, 3}}},
        {{1, 1, 10}, 3, {{0, 1}, {1, 2}, {2, 3}}},  // the first group would take two tasks: one is left for each later group
        {forty, 1, {{0, 40}}},
        {forty, 2, {{0, 20}, {20, 40}}},
        {forty, 3, {{0, 14}, {14, 26}, {26, 40}}},
        {forty, 4, {{0, 9}, {9, 20}, {20, 29}, {29, 40}}},
    };
    for (const Case& k : cases) {
        const int n = (int)k.sizes.size();
        std::vector<int32_t> first(1, 0);
        for (int sz : k.sizes) first.push_back(first.back() + sz);
        const std::vector<std::pair<int, int>> g = lumo::dev::task_groups(first.data(), n, first.back(), k.G);
        CHECK((int)g.size() == k.G);
        CHECK(g.front().first == 0 && g.back().second == n);
        for (int i = 0; i < k.G; ++i) {
            CHECK(g[(size_t)i].second > g[(size_t)i].first);
            if (i) CHECK(g[(size_t)i].first == g[(size_t)i - 1].second);
        }
        CHECK(g == k.want);
    }
}

}  // namespace

int main() {
    plans();
    groups();
    cornell();
    brute();
    textured();
    hostile();
    tasks();
    std::printf("sanitize ok\n");
    return 0;
}
