// check_sac_train_layout -- csrc/dn_internal.h's dn_sac_train_layout and csrc/dn_sac_math.h's dn_polyak on the host, against the rules
// of include/dronenav.h written out independently:
//   over a sweep of (n_nets, layers, head parts, input widths, batch) the scratch regions -- per network h_l and dZ_l per hidden layer,
//   the d_weight partials and the d_bias partials per layer, the head taken as one layer -- are 256-byte aligned, disjoint, in the
//   documented order, network after network, and end at the total that dn_sac_train_scratch_bytes answers;
//   dn_polyak(t, s, tau, 1.0 - tau) is the header's statement -- two float64 products, one float64 add, each correctly rounded, and one
//   rounding to float32 -- evaluated independently in binary128, where both products are exact before their one rounding; for tau in
//   {0, 0.005, 0.5, 1} and drawn ones and a few million pseudo-random (t, s), any two bit patterns and pairs a few ulp apart; it leaves s
//   at tau = 1 and t at tau = 0 bit for bit.  Against the long-double statement omt t + tau s rounded once it is never more than one
//   float32 ulp away; it is not always equal, and cannot be: with tau = 0.005 the exact result sits beside a float32 tie whenever
//   t / 200 is half an ulp of the result (0.995 is 199 / 200 to 2^-55), closer than float64 or the 64-bit long double resolves, and the
//   two round the tie differently.  The count of such pairs is printed ("long_double_differs"), not asserted.
// Prints one JSON line; exit status 0 = all held.
#include "dn_internal.h"
#include "dn_sac_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static long long layouts = 0, polyak = 0, failures = 0, long_double_differs = 0;

static void fail(const char *what, long long a, long long b)
{
    if (failures++ < 10) std::fprintf(stderr, "%s: %lld against %lld\n", what, a, b);
}

static long long r256(long long b) { return (b + 255) / 256 * 256; }

static void check_layout(int n_nets, int n_layers, int parts, const int *in_dims, const int *out_dims, long long batch)
{
    ++layouts;
    const int E = n_layers - 1 + parts;
    dn_mlp_train_layer net[DN_SAC_TRAIN_MAX_ENTRIES];
    std::memset(net, 0, sizeof net);
    for (int l = 0; l < E; ++l) { net[l].in_dim = in_dims[l]; net[l].out_dim = out_dims[l]; }
    const DnSacTrainLayout lay = dn_sac_train_layout(net, n_nets, n_layers, parts, batch);
    // the documented walk: the head as one layer of the parts' outputs together
    int in[DN_MLP_TRAIN_MAX_LAYERS], out[DN_MLP_TRAIN_MAX_LAYERS];
    for (int l = 0; l < n_layers - 1; ++l) { in[l] = in_dims[l]; out[l] = out_dims[l]; }
    in[n_layers - 1] = in_dims[n_layers - 1];
    out[n_layers - 1] = 0;
    for (int p = 0; p < parts; ++p) out[n_layers - 1] += out_dims[n_layers - 1 + p];
    const long long chunks = (batch + DN_MLP_TRAIN_CHUNK - 1) / DN_MLP_TRAIN_CHUNK;
    if (lay.one.chunks != chunks) fail("chunks", lay.one.chunks, chunks);
    long long at = 0;
    for (int c = 0; c < n_nets; ++c) {
        const long long base = c * lay.per_net;
        if (base != at) fail("a network's block does not begin where the one before ends", base, at);
        for (int l = 0; l < n_layers - 1; ++l) {
            if (base + lay.one.h[l] != at) fail("h", base + lay.one.h[l], at);
            at += r256(4 * batch * out[l]);
        }
        for (int l = 0; l < n_layers - 1; ++l) {
            if (base + lay.one.dz[l] != at) fail("dz", base + lay.one.dz[l], at);
            at += r256(4 * batch * out[l]);
        }
        for (int l = 0; l < n_layers; ++l) {
            if (base + lay.one.wpart[l] != at) fail("wpart", base + lay.one.wpart[l], at);
            at += r256(4 * chunks * out[l] * in[l]);
        }
        for (int l = 0; l < n_layers; ++l) {
            if (base + lay.one.bpart[l] != at) fail("bpart", base + lay.one.bpart[l], at);
            at += r256(8 * chunks * out[l]);
        }
    }
    if (at % 256) fail("a region is not 256-byte aligned", at, 0);
    if (lay.total != at) fail("total", lay.total, at);
}

static float from_bits(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits_of(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static void check_polyak(float t, float s, double tau)
{
    if (t != t || s != s || t - t != 0.0f || s - s != 0.0f) return;       // finite pairs only
    ++polyak;
    const double omt = 1.0 - tau;
    const float got = dn_polyak(t, s, tau, omt);
    const double keep = (double)((__float128)omt * (__float128)t), take = (double)((__float128)tau * (__float128)s);
    const float want = (float)(double)((__float128)keep + (__float128)take);
    if (bits_of(got) != bits_of(want) && !(got == 0.0f && want == 0.0f)) fail("polyak", bits_of(got), bits_of(want));
    const float once = (float)((long double)omt * (long double)t + (long double)tau * (long double)s);
    if (bits_of(got) != bits_of(once) && !(got == 0.0f && once == 0.0f)) {
        ++long_double_differs;
        const long long d = (long long)(bits_of(got) & 0x7fffffffu) - (long long)(bits_of(once) & 0x7fffffffu);
        if ((bits_of(got) ^ bits_of(once)) >> 31 || d > 1 || d < -1) fail("polyak is more than one ulp from the long-double statement", bits_of(got), bits_of(once));
    }
    if (tau == 1.0 && got != s) fail("tau = 1 must leave the source", bits_of(got), bits_of(s));
    if (tau == 0.0 && got != t) fail("tau = 0 must leave the target", bits_of(got), bits_of(t));
}

int main(int argc, char **argv)
{
    const long long random = argc > 1 ? std::atoll(argv[1]) : 3000000;
    const long long batches[] = {1, 33, 255, 256, 1023, 1024, 1025, 2053, 65536, 1ll << 24};
    const int widths[] = {32, 96, 256, 512}, firsts[] = {1, 13, 16, 17, 33, 64}, heads[] = {1, 3, 16, 31};
    for (int n_nets = 1; n_nets <= DN_SAC_TRAIN_MAX_NETS; ++n_nets)
        for (int n_layers = 2; n_layers <= DN_MLP_TRAIN_MAX_LAYERS; ++n_layers)
            for (int parts = 1; parts <= DN_SAC_TRAIN_MAX_PARTS; ++parts)
                for (int first : firsts)
                    for (int w : widths)
                        for (int head : heads)
                            for (long long batch : batches) {
                                int in[DN_SAC_TRAIN_MAX_ENTRIES], out[DN_SAC_TRAIN_MAX_ENTRIES];
                                int before = first, width = w;
                                for (int l = 0; l < n_layers - 1; ++l) {
                                    in[l] = before;
                                    out[l] = width;
                                    before = width;
                                    width = width > 32 ? width / 2 / 32 * 32 : 32;     // narrowing, still a multiple of 32
                                }
                                for (int p = 0; p < parts; ++p) {
                                    in[n_layers - 1 + p] = before;
                                    out[n_layers - 1 + p] = p == 0 ? head : 32 - head;
                                }
                                check_layout(n_nets, n_layers, parts, in, out, batch);
                            }
    uint64_t z = 0x9e3779b97f4a7c15ull;
    const double taus[] = {0.0, 0.005, 0.5, 1.0};
    for (long long i = 0; i < random; ++i) {                   // splitmix64
        z += 0x9e3779b97f4a7c15ull;
        uint64_t v = z;
        v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
        v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
        v ^= v >> 31;
        // any two bit patterns and a pair a few ulp apart (a target beside its source), under the four named coefficients and drawn ones
        const float t = from_bits((uint32_t)v);
        const float s = from_bits((uint32_t)(v >> 32));
        const double tau = (i & 7) < 4 ? taus[i & 3] : (double)((v >> 40) & 0xffffff) / 16777216.0;
        check_polyak(t, s, tau);
        check_polyak(s, t, tau);
        const float near = from_bits((uint32_t)v ^ (uint32_t)((v >> 52) & 0xfff));
        check_polyak(t, near, tau);
    }
    std::printf("{\"layouts\": %lld, \"polyak\": %lld, \"long_double_differs\": %lld, \"failures\": %lld}\n", layouts, polyak, long_double_differs, failures);
    return failures ? 1 : 0;
}
