// dn_replay.hip -- SAC replay minibatches on the device for gfx950 (dn_replay_sample, include/dronenav.h).
//
// SB3's ReplayBuffer.sample [from recall]: per output row a slot and a drone (the keyed draw of dn_replay_draw.h, or the caller's flat
// index, clamped), and the row's transition gathered from the [slot][drone] buffers of either layout -- collector.ReplayBuffer's six plain
// arrays, or collector.RingReplayBuffer's ring of T + 1 observation rows with its terminal observations and uint8 flags.
//
// ONE ordinary launch: no workgroup waits for another, no LDS, no atomics, nothing allocated.  The work is some 32 words a row and is
// bound by launches and latency, not bandwidth, so the grid is cut fine and no lane waits for another lane's result:
//   grid (blocks of DN_REPLAY_BLOCK_ROWS = 16 output rows, 3 parts), 256 lanes.  Part 0 writes obs, part 1 next_obs, part 2 the row's
//   tail: actions | reward | dones, act_dim + 2 words.  The lanes walk the block's output words of their part, word q = row q / width,
//   column q % width: the lanes of a wave cover consecutive words of consecutive rows, so stores are fully coalesced and loads coalesced
//   within a row.  Each lane forms its row's transition itself -- the draw is a handful of integer operations on kernel arguments (the
//   key: scalar work, once per wave) -- and then issues its one dependent load.  The lanes of part 1 read the row's done flag (one
//   byte, the same address for the row's lanes) to choose between the terminal observation and the ring's next row; the tail's last lane
//   reads the row's two flags once and forms dones; the tail's reward lane also writes indices_out.
// Every source offset is 64-bit: (T + 1) N D words is not bounded by 2^31.  Rows of 13 words are not 16-byte aligned: 32-bit words.
#include "dn_internal.h"
#include "dn_replay_draw.h"

namespace {

constexpr int RP_THREADS = 256;

// The transition of output row j: the clamped caller's index, or the draw.
__device__ __forceinline__ DnReplayPick rp_pick(const DnReplayArgs &a, const uint64_t key, const unsigned j)
{
    if (a.indices) {
        const long long v = a.indices[j], n = (long long)a.n, q = v / n, r = v - q * n;
        DnReplayPick p;
        p.slot = q < 0 ? 0u : q > (long long)a.t - 1 ? a.t - 1u : (unsigned)q;
        p.env = r < 0 ? 0u : (unsigned)r;              // |r| < n
        return p;
    }
    return dn_replay_draw_at(key, j, a.s, a.n, a.skip);
}

__global__ __launch_bounds__(RP_THREADS) void replay_gather_kernel(const DnReplayArgs a)
{
    const int tid = (int)threadIdx.x, part = (int)blockIdx.y;
    const unsigned row0 = blockIdx.x * (unsigned)DN_REPLAY_BLOCK_ROWS;          // < batch <= 2^31 - 1
    const int nrows = (int)(a.batch - row0 < (unsigned)DN_REPLAY_BLOCK_ROWS ? a.batch - row0 : (unsigned)DN_REPLAY_BLOCK_ROWS);   // >= 1
    const uint64_t key = a.indices ? 0ull : dn_replay_key(a.seed, a.draw + (a.draw_offset ? (unsigned long long)*a.draw_offset : 0ull));
    const int A = a.act_dim, w = part < 2 ? a.obs_dim : A + 2;
    const int units = nrows * w, dr = RP_THREADS / w, dc = RP_THREADS % w;
    const size_t n = a.n;
    int r = tid / w, c = tid % w;
    for (int q = tid; q < units; q += RP_THREADS) {
        const unsigned j = row0 + (unsigned)r;                                 // < batch
        const DnReplayPick p = rp_pick(a, key, j);
        const size_t cell = (size_t)p.slot * n + p.env;                        // < T N
        if (part == 0) {
            reinterpret_cast<uint32_t *>(a.obs)[(size_t)row0 * w + q] = static_cast<const uint32_t *>(a.src.obs)[cell * w + c];
        } else if (part == 1) {
            const uint32_t *from = static_cast<const uint32_t *>(a.src.next_obs) + cell * w;
            if (a.ring && !static_cast<const uint8_t *>(a.src.dones)[cell])
                from = static_cast<const uint32_t *>(a.src.obs) + (cell + n) * w;                  // row slot + 1 <= T of the ring
            reinterpret_cast<uint32_t *>(a.next_obs)[(size_t)row0 * w + q] = from[c];
        } else if (c < A) {
            reinterpret_cast<uint32_t *>(a.actions)[(size_t)j * A + c] = static_cast<const uint32_t *>(a.src.actions)[cell * A + c];
        } else if (c == A) {
            reinterpret_cast<uint32_t *>(a.rewards)[j] = static_cast<const uint32_t *>(a.src.rewards)[cell];
            if (a.indices_out) a.indices_out[j] = (long long)cell;
        } else if (a.ring) {
            const bool done = static_cast<const uint8_t *>(a.src.dones)[cell] != 0, timeout = static_cast<const uint8_t *>(a.src.timeouts)[cell] != 0;
            a.dones[j] = done && !timeout ? 1.0f : 0.0f;
        } else {
            a.dones[j] = static_cast<const float *>(a.src.dones)[cell] * (1.0f - static_cast<const float *>(a.src.timeouts)[cell]);
        }
        r += dr;
        c += dc;
        if (c >= w) { c -= w; ++r; }
    }
}

}  // namespace

hipError_t dn_launch_replay(const DnReplayArgs &a, hipStream_t stream)
{
    if (a.batch < 1 || a.batch > 0x7fffffffu || a.s < 1 || a.n < 1 || a.t < a.s || a.obs_dim < 1 || a.obs_dim > DN_REPLAY_MAX_OBS || a.act_dim < 1 ||
        a.act_dim > DN_REPLAY_MAX_ACT)
        return hipErrorInvalidValue;
    const unsigned blocks = (a.batch - 1u) / (unsigned)DN_REPLAY_BLOCK_ROWS + 1u;
    hipLaunchKernelGGL(replay_gather_kernel, dim3(blocks, 3), dim3(RP_THREADS), 0, stream, a);
    return hipGetLastError();
}
