// dn_history.hip -- observation and action history rows for gfx950 (dn_stack_history, include/dronenav.h).
//
// Pure data movement after the step: every word of a row is a copy of a float32 word of `prev`, `obs`, `terminal_obs`, the caller's
// `actions` or the extras, or zero.  No step kernel knows about it.
//
// Shape: one lane per (drone, 16-byte quad of the row), 256 / (W / 4) drones per workgroup, and the lanes of a drone walk the K steps
// of the launch together with the drone's row in LDS.  A step is the sequential rule itself: every lane reads the up to four words of the
// row of the step before that shift into its quad (13 columns down for an observation frame, 4 for an action frame) from LDS, takes the
// words that are new at this step (the newest observation frame, the newest action frame, the extras) from global memory, stores its
// quad of the step's row with one 16-byte store and puts it into the other LDS buffer for the next step.  So
//   - every input word is read once and every row leaves as contiguous 16-byte stores (a workgroup's drones are neighbours: a step's
//     stores of one workgroup are one contiguous run of up to 4 KiB); `prev` enters the same way;
//   - `prev` may alias any step slot of `rows`: a workgroup owns its drones' rows in every slot, and it has read its drones' whole
//     previous rows (barrier) before its first store;
//   - F, A and E are run-time values: a lane's column map is built once, before the loop, into scalars of its own (no register array is
//     indexed at run time), and the zero frames of an episode start travel through the shifts as the copies they are.
// The 52-byte observation rows and the extras are read as single 4-byte words (they are 4-byte aligned only).
#include "dn_internal.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_MAX_W = 64;

struct HistArgs {
    int frames, actions, extra_dim, width;
    long long k, n;
    const float *prev, *obs, *act, *term_obs, *extra, *term_extra;
    const uint8_t *done;
    float *rows, *term_rows;
};

typedef float hist_v4f __attribute__((ext_vector_type(4)));

// What one word of a lane's quad is made of.  src >= 0: column `src` of the drone's row of the step before.  Otherwise a word that is
// new at every step: fresh[stride * (t * N + drone)] (nullptr: zero), and in a terminal row term[...] in its place.  keep: the word
// survives an episode start (the newest observation frame and the extras; the action frames of a fresh episode are zero).
struct HistWord {
    int src, stride;
    const float *fresh, *term;
    bool keep;
};

__device__ __forceinline__ HistWord hist_word(const HistArgs &a, const int c)
{
    HistWord w{-1, 0, nullptr, nullptr, false};
    const int obs_end = 13 * a.frames, act_end = obs_end + 4 * a.actions;
    if (c < obs_end) {
        if (c + 13 < obs_end) w.src = c + 13;
        else {
            w.fresh = a.obs + (c + 13 - obs_end);
            w.term = a.term_obs ? a.term_obs + (c + 13 - obs_end) : nullptr;
            w.stride = 13;
            w.keep = true;
        }
    } else if (c < act_end) {
        if (c + 4 < act_end) w.src = c + 4;
        else if (a.act) { w.fresh = w.term = a.act + (c + 4 - act_end); w.stride = 4; }
    } else if (c < act_end + a.extra_dim) {
        if (a.extra) w.fresh = a.extra + (c - act_end);
        if (a.term_extra) w.term = a.term_extra + (c - act_end);
        w.stride = a.extra_dim;
        w.keep = true;
    }
    return w;
}

__global__ __launch_bounds__(HIST_THREADS) void dn_history_kernel(const HistArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[2][HIST_THREADS * 4];     // two images of the workgroup's rows, [drone][W]

    const int qw = a.width >> 2;                          // quads per row: 4 .. 16
    const int per = HIST_THREADS / qw;                    // drones per workgroup: 16 .. 64
    const int dl = (int)threadIdx.x / qw, q = (int)threadIdx.x - dl * qw;
    const long long drone = (long long)blockIdx.x * per + dl;
    const bool active = dl < per && drone < a.n;          // the fleet edge, and the lanes beyond per * qw
    const int at = dl * a.width + 4 * q;                  // this lane's quad in an LDS image (active lanes: at + 3 < 1024)

    const HistWord w0 = hist_word(a, 4 * q), w1 = hist_word(a, 4 * q + 1), w2 = hist_word(a, 4 * q + 2), w3 = hist_word(a, 4 * q + 3);

    hist_v4f row = {0.0f, 0.0f, 0.0f, 0.0f};
    if (active && a.prev) row = *reinterpret_cast<const hist_v4f *>(a.prev + drone * a.width + 4 * q);
    if (active) *reinterpret_cast<hist_v4f *>(&lds[0][at]) = row;
    __syncthreads();                                      // every previous row of the workgroup's drones is read: stores may begin

    const auto fresh = [&](const HistWord &w, const long long r) { return active && w.fresh ? w.fresh[r * w.stride] : 0.0f; };
    const auto flag = [&](const long long r) { return active && a.done && a.done[r] != 0; };

    // the new words and the done flag of a step are loaded one step ahead: they depend on nothing the loop carries
    hist_v4f nw = {fresh(w0, drone), fresh(w1, drone), fresh(w2, drone), fresh(w3, drone)};
    bool nd = flag(drone);
    for (long long t = 0; t < a.k; ++t) {
        const long long r = t * a.n + drone;
        const hist_v4f v = nw;
        const bool d = nd;
        if (t + 1 < a.k) {
            nw = hist_v4f{fresh(w0, r + a.n), fresh(w1, r + a.n), fresh(w2, r + a.n), fresh(w3, r + a.n)};
            nd = flag(r + a.n);
        }
        const float *cur = lds[t & 1] + dl * a.width;
        const auto shifted = [&](const HistWord &w) { return active && w.src >= 0 ? cur[w.src] : 0.0f; };
        const hist_v4f old = {shifted(w0), shifted(w1), shifted(w2), shifted(w3)};
        if (d) {
            if (a.term_rows) {
                const auto tw = [&](const HistWord &w, const float o) { return w.src >= 0 ? o : w.term ? w.term[r * w.stride] : 0.0f; };
                *reinterpret_cast<hist_v4f *>(a.term_rows + r * a.width + 4 * q) = hist_v4f{tw(w0, old.x), tw(w1, old.y), tw(w2, old.z), tw(w3, old.w)};
            }
            row = hist_v4f{w0.keep ? v.x : 0.0f, w1.keep ? v.y : 0.0f, w2.keep ? v.z : 0.0f, w3.keep ? v.w : 0.0f};
        } else {
            row = hist_v4f{w0.src >= 0 ? old.x : v.x, w1.src >= 0 ? old.y : v.y, w2.src >= 0 ? old.z : v.z, w3.src >= 0 ? old.w : v.w};
        }
        if (active) {
            *reinterpret_cast<hist_v4f *>(a.rows + r * a.width + 4 * q) = row;
            *reinterpret_cast<hist_v4f *>(&lds[(t + 1) & 1][at]) = row;
        }
        __syncthreads();                                  // the image of step t is whole; the one of step t - 1 is free
    }
}

}  // namespace

hipError_t dn_launch_history(int frames, int actions, int extra_dim, long long k, long long n, const float *prev, const float *obs,
                             const float *act, const uint8_t *done, const float *term_obs, const float *extra, const float *term_extra,
                             float *rows, float *term_rows, hipStream_t stream)
{
    HistArgs a;
    a.frames = frames; a.actions = actions; a.extra_dim = extra_dim; a.width = dn_history_row_width(frames, actions, extra_dim);
    if (a.width < 4 || a.width > HIST_MAX_W) return hipErrorInvalidValue;
    a.k = k; a.n = n;
    a.prev = prev; a.obs = obs; a.act = act; a.term_obs = term_obs; a.extra = extra_dim ? extra : nullptr;
    a.term_extra = extra_dim ? term_extra : nullptr;
    a.done = done; a.rows = rows; a.term_rows = term_rows;
    const long long per = HIST_THREADS / (a.width / 4);
    const long long grid = (n + per - 1) / per;
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_history_kernel, dim3((unsigned)grid), dim3(HIST_THREADS), 0, stream, a);
    return hipGetLastError();
}
