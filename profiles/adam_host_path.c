/* Host time of dn_adam_step's argument checks, two builds side by side; needs no GPU.
 *
 *     gcc -O2 -I include profiles/adam_host_path.c -o /tmp/adam_host_path -ldl
 *     /tmp/adam_host_path OLD/libdronenav.so NEW/libdronenav.so
 *
 * 25 valid tensors, dummy device addresses that are never followed, device_id 2^20: every call passes validation and ends at the
 * failing hipSetDevice.  Both libraries in one process, alternated six times; per turn the best of five times 200 000 calls, ns a call.
 */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include "dronenav.h"

typedef int32_t (*adam_step_fn)(const dn_adam_config *, const dn_adam_tensor *, const double *, double *, double *, void *, int64_t, int32_t,
                                void *);

static double now(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec + 1e-9 * t.tv_nsec;
}

int main(int argc, char **argv)
{
    adam_step_fn f[2];
    if (argc != 3) return 1;
    for (int i = 0; i < 2; ++i) {
        void *h = dlopen(argv[1 + i], RTLD_NOW | RTLD_LOCAL);
        if (!h) { puts(dlerror()); return 1; }
        f[i] = (adam_step_fn)dlsym(h, "dn_adam_step");
    }
    dn_adam_tensor t[DN_ADAM_MAX_TENSORS];
    memset(t, 0, sizeof t);
    for (int i = 0; i < 25; ++i) {
        float **field[] = {&t[i].param, &t[i].grad, &t[i].exp_avg, &t[i].exp_avg_sq};
        for (int j = 0; j < 4; ++j) *field[j] = (float *)(0x10000000ul + 0x100000ul * (unsigned long)(4 * i + j));
        t[i].count = 50000;
    }
    dn_adam_config c;
    memset(&c, 0, sizeof c);
    c.beta1 = 0.9; c.beta2 = 0.999; c.eps = 1e-8; c.max_grad_norm = 0.5; c.n_tensors = 25;
    for (int turn = 0; turn < 6; ++turn)
        for (int i = 0; i < 2; ++i) {
            double best = 1e9;
            for (int r = 0; r < 5; ++r) {
                const double t0 = now();
                int32_t s = 0;
                for (int k = 0; k < 200000; ++k)
                    s += f[i](&c, t, (double *)0x50000000, (double *)0x51000000, (double *)0x52000000, (void *)0x53000000, 1 << 20, 1 << 20, 0);
                const double dt = (now() - t0) / 200000;
                if (dt < best) best = dt;
                if (s == 0) return 2;                  /* a call that returned DN_OK followed a dummy pointer: never here */
            }
            printf("%s %.1f ns\n", i ? "new" : "old", best * 1e9);
        }
    return 0;
}
