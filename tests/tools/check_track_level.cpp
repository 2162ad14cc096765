// check_track_level.cpp -- dn_model_level (csrc/dn_internal.h) with the track bank off and on, for every combination of the six per-drone
// models that check_model_level.cpp walks (144 cases, times two).  Bank off: the level is the deepest model that counts, the rule of
// check_model_level.cpp restated; bank on: DN_M_GOAL, whatever else is on and whatever the goal rows' binding -- the bank rides in that
// family and has no level of its own.  Host only: no HIP call, no GPU.  Prints one JSON line; the exit status is 1 if a case is wrong.
#include <cstdio>

#include "dn_internal.h"

static_assert(DN_M_GOAL == 6 && DN_M_COUNT == 7, "the bank adds no level");

int main()
{
    static float4 quad;
    static float row;
    static int word;
    static double cdf;
    static unsigned long long count[5];
    int cases = 0, bad = 0;
    for (int bank = 0; bank < 2; ++bank)
        for (int dyn = 0; dyn < 2; ++dyn)
            for (int wind = 0; wind < 2; ++wind)
                for (int act = 0; act < 2; ++act)
                    for (int sens = 0; sens < 2; ++sens)
                        for (int priv = 0; priv < 3; ++priv)            // 0 off, 1 enabled and unbound, 2 enabled and bound
                            for (int goal = 0; goal < 3; ++goal) {
                                DnModels m = {};
                                if (dyn) m.dyn.dyn = &quad;
                                if (wind) { m.wind.mean = &quad; m.wind.gust = &quad; }
                                if (act) { m.act.hist = &quad; m.act.rpm = &quad; m.act.coeff = &row; m.act.lat = &word; }
                                if (sens) { m.sens.ring = &quad; m.sens.bias = &quad; m.sens.lat = &word; }
                                if (priv) m.priv.groups = DN_PRIV_OBS;
                                if (priv == 2) { m.priv.rows = &row; m.priv.cap = 1; }
                                if (goal) m.goal.on = 1;
                                if (goal == 2) { m.goal.rows = &row; m.goal.cap = 1; }
                                if (bank) {
                                    m.track.track = &word; m.track.finished = &word; m.track.cdf = &cdf; m.track.bw = &word;
                                    m.track.count = count; m.track.num_tracks = 1; m.track.total = 1;
                                }
                                const bool counts[6] = {dyn != 0, wind != 0, act != 0, sens != 0, priv == 2, goal == 2};
                                int want = 0;
                                for (int k = 0; k < 6; ++k)
                                    if (counts[k]) want = k + 1;
                                if (bank) want = DN_M_GOAL;
                                const int got = dn_model_level(m);
                                ++cases;
                                if (got != want) {
                                    ++bad;
                                    fprintf(stderr, "bank %d dyn %d wind %d act %d sens %d priv %d goal %d: level %d, want %d\n", bank, dyn, wind, act,
                                            sens, priv, goal, got, want);
                                }
                            }
    printf("{\"cases\": %d, \"bad\": %d}\n", cases, bad);
    return bad != 0;
}
