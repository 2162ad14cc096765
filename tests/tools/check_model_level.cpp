// check_model_level.cpp -- dn_model_level (csrc/dn_internal.h) against the rule it implements, for every combination of the six per-drone
// models: dynamics, wind, actuator and sensor on or off, privileged and goal rows off / enabled but unbound / enabled and bound (144 cases).
// Host only: no HIP call, no GPU.  Prints one JSON line; the exit status is the number of wrong cases (capped at 1).
#include <cstdio>

#include "dn_internal.h"

static_assert(DN_M_NONE == 0 && DN_M_DYN == 1 && DN_M_WIND == 2 && DN_M_ACT == 3 && DN_M_SENS == 4 && DN_M_PRIV == 5 && DN_M_GOAL == 6 &&
                  DN_M_COUNT == 7,
              "the chain, shallowest first");

int main()
{
    static float4 quad;
    static float row;
    static int word;
    int cases = 0, bad = 0;
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
                            // the rule, written from the shallow end: the level of the deepest model that counts, none = 0
                            const bool counts[6] = {dyn != 0, wind != 0, act != 0, sens != 0, priv == 2, goal == 2};
                            int want = 0;
                            for (int k = 0; k < 6; ++k)
                                if (counts[k]) want = k + 1;
                            const int got = dn_model_level(m);
                            ++cases;
                            if (got != want) {
                                ++bad;
                                fprintf(stderr, "dyn %d wind %d act %d sens %d priv %d goal %d: level %d, want %d\n", dyn, wind, act, sens, priv, goal,
                                        got, want);
                            }
                        }
    printf("{\"cases\": %d, \"bad\": %d}\n", cases, bad);
    return bad != 0;
}
