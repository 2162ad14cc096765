// dn_argcheck.h -- the argument checks that the entry points of the C ABI share, stated once: byte-range overlap, required pointers,
// alignment, scratch size.  Host-only and without HIP: the functions answer, the caller words the refusal (dn_capi_fail.h).
// tests/tools/check_argcheck.cpp walks them against the rules written out independently, plainly and under the sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

// Do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  Never with a null pointer and never with a range of zero bytes.  The ends are
// formed in uintptr_t and may wrap: a range that ends exactly at the top of the address space (end == 0) overlaps nothing, and one
// that runs past it is taken to end at the wrapped address.  No device allocation lies there; the arithmetic is kept as the entry
// points have always had it, so that the answer for every pair of addresses is the one callers have seen.
static inline bool dn_ranges_overlap(const void *a, uintptr_t a_bytes, const void *b, uintptr_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// scratch_bytes against what the entry point's dn_X_scratch_bytes gives
static inline bool dn_scratch_short(int64_t have, int64_t need) { return have < need; }

// One pointer argument of an entry point: its name in the messages, the bytes the call touches behind it, and whether NULL is allowed.
struct DnArg {
    const char *name;
    const void *p;
    uintptr_t bytes;
    bool optional;
};

// The first required pointer that is NULL, or nullptr.
static inline const DnArg *dn_first_missing(const DnArg *args, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!args[i].p && !args[i].optional) return &args[i];
    return nullptr;
}

// The first pointer with a bit of `mask` set (alignment - 1), or nullptr.  NULL is aligned.
static inline const DnArg *dn_first_misaligned(const DnArg *args, size_t n, uintptr_t mask)
{
    for (size_t i = 0; i < n; ++i)
        if ((uintptr_t)args[i].p & mask) return &args[i];
    return nullptr;
}

// The first (output, input) pair that overlaps, outputs in the outer loop; false when there is none.
static inline bool dn_first_overlap(const DnArg *out, size_t n_out, const DnArg *in, size_t n_in, const DnArg **o, const DnArg **i)
{
    for (size_t a = 0; a < n_out; ++a)
        for (size_t b = 0; b < n_in; ++b)
            if (dn_ranges_overlap(out[a].p, out[a].bytes, in[b].p, in[b].bytes)) {
                *o = &out[a];
                *i = &in[b];
                return true;
            }
    return false;
}

// the same walks over a whole array
template <size_t N> static inline const DnArg *dn_first_missing(const DnArg (&args)[N]) { return dn_first_missing(args, N); }
template <size_t N> static inline const DnArg *dn_first_misaligned(const DnArg (&args)[N], uintptr_t mask) { return dn_first_misaligned(args, N, mask); }
template <size_t NO, size_t NI>
static inline bool dn_first_overlap(const DnArg (&out)[NO], const DnArg (&in)[NI], const DnArg **o, const DnArg **i)
{
    return dn_first_overlap(out, NO, in, NI, o, i);
}
