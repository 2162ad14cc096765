// dn_pick_shapes (csrc/dn_shapes.h), the kernel-shape pick of dn_create, over its whole domain.  Host code only: dn_shapes.h is the one
// project header included.
//
// Without arguments: the walk.  Prints {"cases": n, "digest": "<16 hex digits>", "bad": b}; exit status 1 when b > 0.  `cases` counts the
// picks of the walk, `digest` is FNV-1a 64 over their (fused, single) byte pairs in walk order, `bad` counts the walk's pairs of fleet
// sizes that disagree plus the spot rows (below) that do not hold.  The walk, outermost loop first:
//   1. the 144 configuration classes: the base (dn_config_default's literals with ground_contact set explicitly) in twelve variants --
//      as it is, clip_rew = 1, norm_rew = 1, physics = 1, physics = 2, action_type = 1, 2, 3, 4, 5, random_spawn = 1, zero_damping = 1 --
//      each with normalize_obs 0, 1; each with noise none, act_noise_sigma = 0.01, obs_noise_sigma = 0.01; each with ground_contact 0, 1;
//   2. per class first num_cus 1, 8, 32, 64, 256, 304 without overrides, then num_cus 32, 256 with DN_WAVES in {unset, "", "0", "1", "2",
//      "3", "4", "5", "8", "9", "3x"} (outer) x DN_WAVES_SINGLE in {unset, "1", "2", "3"} (inner);
//   3. blocks 1 .. 8 num_cus + 2;
//   4. num_envs = 64 blocks, then 64 (blocks - 1) + 1: the two picks must agree.
// The spot rows are written out by hand from the measurement notes of dn_shapes.h and from _expected_fused_waves of
// tests/test_gpu_parity.py, not computed by the function under test.
//
// With arguments key=value (num_cus, num_envs, normalize_obs, ground_contact, clip_rew, norm_rew, physics, action_type, random_spawn,
// zero_damping, act_noise_sigma, obs_noise_sigma, dn_waves, dn_waves_single; what is not named keeps the base's value, num_cus 256,
// no overrides): prints the one pick as {"fused": f, "single": s}.
#include "dn_shapes.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static dn_config base_config()
{   // dn_config_default (csrc/dn_capi.cpp), with ground_contact resolved
    dn_config c;
    std::memset(&c, 0, sizeof c);
    c.num_envs = 1;
    c.threshold = 0.3;
    c.max_steps = 4096;
    c.cylinder = 1;
    c.include_distance = 1;
    c.normalize_actions = 1;
    c.ground_contact = 0;
    c.aviary_dim[0] = c.aviary_dim[1] = -1.0;
    c.aviary_dim[3] = c.aviary_dim[4] = c.aviary_dim[5] = 1.0;
    return c;
}

static dn_config variant(int v)
{
    dn_config c = base_config();
    switch (v) {
    case 0: break;
    case 1: c.clip_rew = 1; break;
    case 2: c.norm_rew = 1; break;
    case 3: c.physics = 1; break;
    case 4: c.physics = 2; break;
    case 5: c.action_type = 1; break;
    case 6: c.action_type = 2; break;
    case 7: c.action_type = 3; break;
    case 8: c.action_type = 4; break;
    case 9: c.action_type = 5; break;
    case 10: c.random_spawn = 1; break;
    default: c.zero_damping = 1; break;
    }
    return c;
}
constexpr int NUM_VARIANTS = 12;

static dn_config config_class(int v, int norm, int noise, int ground)
{
    dn_config c = variant(v);
    c.normalize_obs = norm;
    if (noise == 1) c.act_noise_sigma = 0.01f;
    if (noise == 2) c.obs_noise_sigma = 0.01f;
    c.ground_contact = ground;
    return c;
}

static long long g_cases = 0, g_bad = 0;
static uint64_t g_digest = 0xcbf29ce484222325ull;

static void digest_byte(int b)
{
    g_digest ^= (uint64_t)(unsigned char)b;
    g_digest *= 0x100000001b3ull;
}

static DnShapes pick(dn_config c, long long num_envs, int cus, const char *w, const char *ws)
{
    c.num_envs = num_envs;
    return dn_pick_shapes(c, cus, w, ws);
}

// every fleet of 1 .. 8 cus + 2 tiles, a full last tile and a last tile of one drone
static void walk_fleets(const dn_config &c, int cus, const char *w, const char *ws)
{
    for (long long blocks = 1; blocks <= 8ll * cus + 2; ++blocks) {
        const DnShapes full = pick(c, 64 * blocks, cus, w, ws), one = pick(c, 64 * (blocks - 1) + 1, cus, w, ws);
        digest_byte(full.fused); digest_byte(full.single);
        digest_byte(one.fused); digest_byte(one.single);
        g_cases += 2;
        if (full.fused != one.fused || full.single != one.single) {
            ++g_bad;
            std::fprintf(stderr, "%d CUs, %lld tiles: %d / %d with a full last tile, %d / %d with one drone in it\n", cus, blocks, full.fused, full.single,
                         one.fused, one.single);
        }
    }
}

static const char *shown(const char *s) { return s ? s : "(unset)"; }

// single < 0: the row states the fused pick only
static void expect(const char *what, const dn_config &c, long long num_envs, int cus, const char *w, const char *ws, int fused, int single)
{
    const DnShapes got = pick(c, num_envs, cus, w, ws);
    if (got.fused == fused && (single < 0 || got.single == single)) return;
    ++g_bad;
    std::fprintf(stderr, "%s, %lld drones, %d CUs, DN_WAVES %s, DN_WAVES_SINGLE %s: %d / %d, want %d / %d\n", what, num_envs, cus, shown(w), shown(ws),
                 got.fused, got.single, fused, single);
}

static void spot_rows()
{
    const dn_config plain = base_config();
    dn_config norm = plain, ground = plain, act_noise = plain, clip = plain, pid = plain, spawn = plain;
    norm.normalize_obs = 1;
    ground.ground_contact = 1;
    act_noise.act_noise_sigma = 0.01f;
    clip.clip_rew = 1;
    pid.action_type = 2;
    spawn.random_spawn = 1;
    // 256 CUs, no overrides
    expect("plain", plain, 32768, 256, nullptr, nullptr, 4, 3);
    expect("plain", plain, 49152, 256, nullptr, nullptr, 4, 3);
    expect("plain", plain, 65536, 256, nullptr, nullptr, 3, 3);
    expect("plain", plain, 65600, 256, nullptr, nullptr, 1, 1);
    expect("normaliser", norm, 4096, 256, nullptr, nullptr, 8, 3);
    expect("normaliser", norm, 16384, 256, nullptr, nullptr, 8, 3);
    expect("normaliser", norm, 32768, 256, nullptr, nullptr, 5, 3);
    expect("normaliser", norm, 32832, 256, nullptr, nullptr, 4, 1);
    expect("normaliser", norm, 49152, 256, nullptr, nullptr, 4, 1);
    expect("normaliser", norm, 65536, 256, nullptr, nullptr, 8, 1);
    expect("normaliser", norm, 98304, 256, nullptr, nullptr, 8, 1);
    expect("normaliser", norm, 131072, 256, nullptr, nullptr, 1, 1);
    expect("ground contact", ground, 65536, 256, nullptr, nullptr, 3, 1);
    expect("action noise", act_noise, 32768, 256, nullptr, nullptr, 4, 3);
    expect("action noise", act_noise, 49152, 256, nullptr, nullptr, 2, 3);
    expect("clip_rew", clip, 49152, 256, nullptr, nullptr, 3, -1);
    expect("clip_rew", clip, 65536, 256, nullptr, nullptr, 2, -1);
    expect("clip_rew", clip, 65600, 256, nullptr, nullptr, 1, -1);
    // at every fleet size of the grid
    const int all_cus[] = {1, 8, 32, 64, 256, 304};
    for (int cus : all_cus)
        for (long long blocks = 1; blocks <= 8ll * cus + 2; ++blocks) {
            const long long n = 64 * blocks;
            expect("action_type 2", pid, n, cus, nullptr, nullptr, 1, 1);
            expect("action_type 2", pid, n, cus, "8", nullptr, 1, 1);
            expect("random_spawn", spawn, n, cus, nullptr, nullptr, 1, 1);
            expect("normaliser", norm, n, cus, "2", nullptr, 2, 2);
            for (int v = 0; v < NUM_VARIANTS; ++v)
                for (int on = 0; on < 2; ++on) {
                    const dn_config c = config_class(v, on, 0, 0);
                    const DnShapes three = pick(c, n, cus, "3", nullptr);
                    expect("DN_WAVES=3x as DN_WAVES=3", c, n, cus, "3x", nullptr, three.fused, three.single);
                }
        }
}

static int print_one(int argc, char **argv)
{
    dn_config c = base_config();
    int cus = (int)DN_CALIBRATION_CUS;
    const char *w = nullptr, *ws = nullptr;
    for (int k = 1; k < argc; ++k) {
        const char *eq = std::strchr(argv[k], '=');
        if (!eq) { std::fprintf(stderr, "%s: expected key=value\n", argv[k]); return 2; }
        const size_t len = (size_t)(eq - argv[k]);
        const char *val = eq + 1;
        const auto is = [&](const char *key) { return std::strlen(key) == len && std::strncmp(argv[k], key, len) == 0; };
        if (is("num_cus")) cus = std::atoi(val);
        else if (is("num_envs")) c.num_envs = std::atoll(val);
        else if (is("normalize_obs")) c.normalize_obs = std::atoi(val);
        else if (is("ground_contact")) c.ground_contact = std::atoi(val);
        else if (is("clip_rew")) c.clip_rew = std::atoi(val);
        else if (is("norm_rew")) c.norm_rew = std::atoi(val);
        else if (is("physics")) c.physics = std::atoi(val);
        else if (is("action_type")) c.action_type = std::atoi(val);
        else if (is("random_spawn")) c.random_spawn = std::atoi(val);
        else if (is("zero_damping")) c.zero_damping = std::atoi(val);
        else if (is("act_noise_sigma")) c.act_noise_sigma = (float)std::atof(val);
        else if (is("obs_noise_sigma")) c.obs_noise_sigma = (float)std::atof(val);
        else if (is("dn_waves")) w = val;
        else if (is("dn_waves_single")) ws = val;
        else { std::fprintf(stderr, "%s: unknown key\n", argv[k]); return 2; }
    }
    if (cus < 1 || c.num_envs < 1) { std::fprintf(stderr, "num_cus and num_envs must be >= 1\n"); return 2; }
    const DnShapes s = dn_pick_shapes(c, cus, w, ws);
    std::printf("{\"fused\": %d, \"single\": %d}\n", s.fused, s.single);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) return print_one(argc, argv);
    const int all_cus[] = {1, 8, 32, 64, 256, 304}, override_cus[] = {32, 256};
    const char *const waves[] = {nullptr, "", "0", "1", "2", "3", "4", "5", "8", "9", "3x"};
    const char *const waves_single[] = {nullptr, "1", "2", "3"};
    for (int v = 0; v < NUM_VARIANTS; ++v)
        for (int norm = 0; norm < 2; ++norm)
            for (int noise = 0; noise < 3; ++noise)
                for (int ground = 0; ground < 2; ++ground) {
                    const dn_config c = config_class(v, norm, noise, ground);
                    for (int cus : all_cus) walk_fleets(c, cus, nullptr, nullptr);
                    for (int cus : override_cus)
                        for (const char *w : waves)
                            for (const char *ws : waves_single) walk_fleets(c, cus, w, ws);
                }
    spot_rows();
    std::printf("{\"cases\": %lld, \"digest\": \"%016llx\", \"bad\": %lld}\n", g_cases, (unsigned long long)g_digest, g_bad);
    return g_bad ? 1 : 0;
}
