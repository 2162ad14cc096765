// dn_mlp_ks1 (csrc/dn_internal.h): the layer-1 K-steps a PPO policy kernel runs for rows of obs_dim columns, over obs_dim = -1 .. 70,
// against the rule written out independently of the function: refuse (0) outside 1..64, else ceil(obs_dim / 16) rounded up to a power of
// two (there is no three-K-step kernel).  Prints {"cases": n, "bad": b}; exit status 1 when b > 0.  Host code only.
#include "dn_internal.h"

#include <cstdio>

int main()
{
    int cases = 0, bad = 0;
    for (int d = -1; d <= 70; ++d) {
        int want = 0;
        if (d >= 1 && d <= 64) {
            const int steps = (d + 15) / 16;                // 1 .. 4
            want = 1;
            while (want < steps) want *= 2;
        }
        const int got = dn_mlp_ks1(d);
        if (got != want) {
            ++bad;
            std::fprintf(stderr, "obs_dim %d: dn_mlp_ks1 = %d, want %d\n", d, got, want);
        }
        ++cases;
    }
    std::printf("{\"cases\": %d, \"bad\": %d}\n", cases, bad);
    return bad ? 1 : 0;
}
