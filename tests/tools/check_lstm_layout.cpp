// check_lstm_layout -- csrc/dn_internal.h's dn_lstm_layout and dn_lstm_prev on the host, against the rules of include/dronenav.h
// written out independently, over a sweep of (I, H, T, B):
//   the scratch regions -- the gates, carry_h, carry_c, the weight-gradient partials, the bias partials -- are 256-byte aligned,
//   disjoint, in the documented order, and end at the total that dn_lstm_scratch_bytes answers; the forward's share is the gates alone;
//   row t B + b of hprev comes from nowhere where the row's episode starts at t, else from row b of h0 at t = 0 and from row
//   (t - 1) B + b of h_seq later -- walked row by row with the rows on both sides of every chunk edge of DN_MLP_TRAIN_CHUNK rows, which
//   fall inside a step whenever B is not a divisor of the chunk, and held against a [T][B] table built step by step.
// Prints one JSON line; exit status 0 = all held.
#include "dn_internal.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static long long layouts = 0, rows_checked = 0, straddling = 0, failures = 0;

static void fail(const char *what, long long a, long long b)
{
    if (failures++ < 10) std::fprintf(stderr, "%s: %lld against %lld\n", what, a, b);
}

static long long r256(long long b) { return (b + 255) / 256 * 256; }

static void check_layout(int I, int H, long long T, long long B)
{
    ++layouts;
    const DnLstmLayout lay = dn_lstm_layout(I, H, T, B);
    const long long chunks = (T * B + DN_MLP_TRAIN_CHUNK - 1) / DN_MLP_TRAIN_CHUNK;
    if (lay.chunks != chunks) fail("chunks", lay.chunks, chunks);
    const long long offsets[] = {lay.gates, lay.carry_h, lay.carry_c, lay.wpart, lay.bpart};
    const long long sizes[] = {r256(16 * T * B * H), r256(4 * B * H), r256(4 * B * H), r256(16 * chunks * H * (I + H)), r256(32 * chunks * H)};
    const long long used[] = {4 * T * B * 4 * H, 4 * B * H, 4 * B * H, 4 * chunks * 4 * H * (I + H), 8 * chunks * 4 * H};
    long long at = 0;
    for (int k = 0; k < 5; ++k) {
        if (offsets[k] != at) fail("a region does not begin where the one before ends", offsets[k], at);
        if (offsets[k] % 256) fail("a region is not 256-byte aligned", offsets[k], k);
        if (used[k] > sizes[k]) fail("a region is smaller than what is kept in it", sizes[k], used[k]);
        at += sizes[k];
    }
    if (lay.total != at) fail("total", lay.total, at);
    if (lay.carry_h != r256(16 * T * B * H)) fail("the forward's share is the gates", lay.carry_h, r256(16 * T * B * H));
}

// the rule, stated over (t, b): source 0 none, 1 h0 row b, 2 h_seq row (t - 1) B + b
static void check_row(long long row, long long T, long long B, const std::vector<unsigned char> &starts)
{
    ++rows_checked;
    const long long t = row / B, b = row % B;
    const int start = starts[(size_t)row];
    const DnLstmPrev got = dn_lstm_prev(row, B, start);
    int source = 2;
    long long want = (t - 1) * B + b;
    if (t == 0) { source = 1; want = b; }
    if (start) { source = 0; want = 0; }
    if (got.source != source) fail("source", got.source, source);
    if (got.row != want) fail("row", got.row, want);
    if (source == 1 && (got.row < 0 || got.row >= B)) fail("a row of h0 out of range", got.row, B);
    if (source == 2 && (got.row < 0 || got.row >= (T - 1) * B)) fail("a row of h_seq at or beyond the step before the last", got.row, (T - 1) * B);
}

static void check_rows(long long T, long long B, uint64_t &z)
{
    std::vector<unsigned char> starts((size_t)(T * B));
    for (auto &s : starts) {                            // splitmix64: one cell in five starts an episode
        z += 0x9e3779b97f4a7c15ull;
        uint64_t v = z;
        v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
        v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
        s = (v ^ (v >> 31)) % 5 == 0;
    }
    const long long rows = T * B;
    if (rows <= 8192) {
        for (long long row = 0; row < rows; ++row) check_row(row, T, B, starts);
    } else {                                            // the first and last steps, and both sides of every chunk edge
        for (long long row = 0; row < 2 * B && row < rows; ++row) check_row(row, T, B, starts);
        for (long long row = rows - B; row < rows; ++row) check_row(row, T, B, starts);
    }
    for (long long edge = DN_MLP_TRAIN_CHUNK; edge < rows; edge += DN_MLP_TRAIN_CHUNK) {
        if (edge % B) ++straddling;                     // the chunk edge falls inside a step
        check_row(edge - 1, T, B, starts);
        check_row(edge, T, B, starts);
    }
}

int main()
{
    const int ins[] = {1, 13, 17, 33, 64}, hiddens[] = {32, 64, 96, 160, 256, 512};
    const long long steps[] = {1, 2, 3, 5, 32, 1024}, batches[] = {1, 31, 33, 129, 205, 683, 1024, 1025, 4096, 16384, 1ll << 24};
    uint64_t z = 0x9e3779b97f4a7c15ull;
    for (long long T : steps)
        for (long long B : batches) {
            if (T * B > (1ll << 24)) continue;
            for (int I : ins)
                for (int H : hiddens) check_layout(I, H, T, B);
            if (T * B <= (1ll << 20)) check_rows(T, B, z);
        }
    std::printf("{\"layouts\": %lld, \"rows\": %lld, \"straddling_edges\": %lld, \"failures\": %lld}\n", layouts, rows_checked, straddling, failures);
    return failures ? 1 : 0;
}
