// dn_second_moment.h -- the observation normaliser's second moment across the state blob (dn_get_state / dn_set_state).
//
// Standard C++ only, host code: dn_capi.cpp calls dn_restore_second_moment per column in dn_set_state, and
// tests/tools/check_second_moment.cpp walks the functions below over more than a million (M2, count) pairs on the CPU.
//
// The device carries M2 = RunningMeanStd.var x .count (dn_internal.h rms_m2); dn_env_state shows var = M2 / count AND, since ABI 10,
// the word M2 itself (rms_m2).  "Reads back as the same var" is not "is the same M2": two neighbouring doubles can divide to the same
// var, so a blob that carried var alone came back with M2 one ulp off for about one word in eleven (profiles/NOTES.md).
#ifndef DN_SECOND_MOMENT_H
#define DN_SECOND_MOMENT_H

#include <cmath>

// The counts dn_set_state takes: positive and finite (RunningMeanStd starts at 1e-4).  Zero, a negative count, NaN and an infinity are
// refused there: M2 / count would not be a variance.
inline bool dn_rms_count_ok(double count) { return count > 0.0 && std::isfinite(count); }

// The second moment for a given RunningMeanStd.var / .count when the word itself is not known -- the double m nearest to var x count
// with m / count == var where one exists (where one exists it is var x count rounded or a neighbour of it: the m that divide to var
// span at most two ulp around var x count), so that dn_get_state of what was just set returns the var it was given.  NOT an inverse
// of M2 -> M2 / count: that map is many to one.
inline double second_moment(double var, double count)
{
    const double m = var * count;
    if (!(count > 0.0) || !std::isfinite(m) || m / count == var) return m;
    const double lo = std::nextafter(m, -HUGE_VAL), hi = std::nextafter(m, HUGE_VAL);
    if (lo / count == var) return lo;
    if (hi / count == var) return hi;
    return m;
}

// THE rule of dn_set_state, per column: m2_hint (dn_env_state.rms_m2) verbatim while it still belongs to the var and count beside it
// -- count > 0, the hint finite, m2_hint / count == var: what dn_get_state wrote, so a blob restores the device word bit for bit.
// Otherwise the caller edited var or count, or the blob comes from a producer that does not fill the hint (zeros): the var given is
// what the next observation is normalised with, through second_moment.
inline double dn_restore_second_moment(double var, double count, double m2_hint)
{
    if (count > 0.0 && std::isfinite(m2_hint) && m2_hint / count == var) return m2_hint;
    return second_moment(var, count);
}

#endif
