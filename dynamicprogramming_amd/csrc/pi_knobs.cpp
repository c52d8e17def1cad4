// pi_knobs.cpp — the table of the PI_MI355_* environment knobs and the only std::getenv calls of csrc/ (pi_knobs.h).

#include "pi_knobs.h"

#include <algorithm>
#include <cassert>
#include <climits>
#include <cstdlib>

namespace pi {
namespace {

// The parse rule of a knob.  They differ for historical reasons and are kept as they are; `e` is the variable's value.
enum class KnobKind {
    Int,        // atoi(e) when it lies in [lo, hi] (text that is no number reads as 0); the default otherwise and when unset
    Block,      // Int, and a value that is no multiple of 64 gives the default too
    Present,    // set to ANY value, "0" and "" included: on; unset: off
    OffIfZero,  // atoi(e) == 0 (so "0", "" and text that is no number): off; any other value or unset: on
    TriState,   // unset: the library decides; atoi(e) == 0: off; any other value: on
    Clamp,      // atoi(e) clamped to [lo, the call's upper limit]; unset: the upper limit
    Count,      // the WHOLE string a decimal integer in [0, the call's upper limit]; anything else or unset: the library decides
    Seconds     // atof(e) when it is positive; the default otherwise
};

constexpr int kGridDefault = -1;      // `dflt` of a row whose default depends on the grid: the call site passes it

// lo, hi: the accepted range of Int and Block, the lower limit of Clamp; doc: the line INTEGRATION.md repeats
struct KnobRow { Knob id; const char* name; KnobKind kind; double dflt; int lo, hi; const char* doc; };
using K = Knob;
using T = KnobKind;

constexpr KnobRow kKnobs[(int)Knob::kCount] = {
    // launch geometry
    {K::EVAL_BLOCK, "PI_MI355_EVAL_BLOCK", T::Block, kGridDefault, 256, 1024, "threads per evaluation workgroup: a multiple of 64 in 256..1024; default 1024 on grids of up to 4-D with >= 2^24 states, else 256; read at pi_create"},
    {K::IMPROVE_BLOCK, "PI_MI355_IMPROVE_BLOCK", T::Block, kGridDefault, 256, 1024, "threads per improvement workgroup: a multiple of 64 in 256..1024; default 512 on grids of up to 4-D with >= 2^24 states, else 256; read at pi_create"},
    {K::EVAL_CPW, "PI_MI355_EVAL_CPW", T::Int, kGridDefault, 1, 64, "chunks per evaluation workgroup, 1..64; default 4 on 6-D grids with >= 2^24 states, else 2 from 2^20 states, else 1; read at pi_create"},
    {K::IMPROVE_CPW, "PI_MI355_IMPROVE_CPW", T::Int, kGridDefault, 1, 64, "chunks per improvement workgroup, 1..64; default 3 on 6-D grids with >= 2^24 states, else 1; read at pi_create"},
    {K::STRIP, "PI_MI355_STRIP", T::Count, -1, 0, 0, "strip schedule: states per period, a whole decimal number in 0..n_states (0 = slab schedule); anything else or unset = the library's choice; read at pi_create"},
    // dispatch
    {K::GRAPHS, "PI_MI355_GRAPHS", T::Int, 1, 0, 1, "0 = launch evaluation batches eagerly instead of replaying a graph; default 1; read at pi_create"},
    {K::RESIDENT, "PI_MI355_RESIDENT", T::Int, 1, 0, 1, "0 = no one-launch kernel at all (LDS-resident, dataflow, XCD-local); default 1; read at pi_create"},
    {K::XCD, "PI_MI355_XCD", T::Int, 1, 0, 1, "0 = no XCD-local kernel (the dataflow and LDS-resident kernels stay); default 1; read at pi_create"},
    // one-launch kernels
    {K::XCD_TIMEOUT, "PI_MI355_XCD_TIMEOUT", T::Seconds, 0.25, 0, 0, "seconds a wave of the XCD-local kernel waits for another: a positive number; default 0.25; read at every launch"},
    {K::FLOW_TIMEOUT, "PI_MI355_FLOW_TIMEOUT", T::Seconds, 2.0, 0, 0, "seconds a wave of the dataflow kernel waits for another: a positive number; default 2; read at every launch"},
    // live lists
    {K::LIVE, "PI_MI355_LIVE", T::Int, 1, 0, 1, "0 = pi_prepare_mask keeps no list of live states; default 1; read at every pi_prepare_mask"},
    {K::LIVE_MIN, "PI_MI355_LIVE_MIN", T::Int, 1 << 20, 1, 1 << 30, "smallest grid (states, 1..2^30) that keeps a live-state list; default 2^20; read at every pi_prepare_mask"},
    {K::EVAL_LIST, "PI_MI355_EVAL_LIST", T::Int, 1, 0, 1, "0 = pi_eval_begin builds no per-evaluation list; default 1; read at every pi_eval_begin"},
    // sharding
    {K::COMM_TIMEOUT, "PI_MI355_COMM_TIMEOUT", T::Seconds, 120.0, 0, 0, "seconds a rank waits for a peer: a positive number; default 120; read at every host wait and at pi_comm_init_p2p"},
    {K::P2P_FUSED, "PI_MI355_P2P_FUSED", T::OffIfZero, 1, 0, 0, "0 = the peer-to-peer exchange copies instead of delivering from inside the sweep: off when the value's leading integer is 0 or it has none, on otherwise and when unset; read at plan time"},
    {K::PAIR_REACH, "PI_MI355_PAIR_REACH", T::OffIfZero, 1, 0, 0, "0 = the fused exchange does not measure the pair reach: off and on as PI_MI355_P2P_FUSED; read at plan time"},
    {K::ROW_EXACT, "PI_MI355_ROW_EXACT", T::TriState, -1, 0, 0, "row-exact and state-exact lists of a plan: 0 = never, any other number = row-exact lists always, unset = where they pay; read at plan time"},
    {K::REACH_DEPTH, "PI_MI355_REACH_DEPTH", T::Clamp, -1, 1, 0, "leading dimensions the reach of a plan is measured in, clamped to 1..pi_reach_depth_max; default the maximum; read at plan time"},
    // debug
    {K::IEEE_DIV, "PI_MI355_IEEE_DIV", T::Present, 0, 0, 0, "set to ANY value (0 included) = IEEE division in every dimension instead of the checked reciprocal; default unset; read at pi_create"},
    {K::DEBUG, "PI_MI355_DEBUG", T::Int, 0, 0, 1, "1 = checked kernels (pi_debug_report); default 0; read at pi_create"},
    {K::DEBUG_DROP_DELIVERY, "PI_MI355_DEBUG_DROP_DELIVERY", T::Int, 0, 1, INT_MAX, "k >= 1 = fault injection for the tests: every k-th delivery of a fused plan is dropped; default 0 (none); read at plan time"},
};

constexpr bool rows_in_enum_order(int i = 0) { return i == (int)Knob::kCount || ((int)kKnobs[i].id == i && rows_in_enum_order(i + 1)); }
static_assert(rows_in_enum_order(), "kKnobs has one row per Knob, in the enum's order");

const KnobRow& row(Knob k) { return kKnobs[(int)k]; }
const char* value(Knob k) { return std::getenv(row(k).name); }

}  // namespace

int knob_int(Knob k, int dflt) {
    const KnobRow& r = row(k);
    if (const char* e = value(k)) {
        const int v = std::atoi(e);
        if (v >= r.lo && v <= r.hi && (r.kind != KnobKind::Block || v % 64 == 0)) return v;
    }
    return dflt;
}
int knob_int(Knob k) {
    assert(row(k).dflt != kGridDefault && "this knob's default depends on the grid: pass it");
    return knob_int(k, (int)row(k).dflt);
}

int knob_flag(Knob k) {
    const char* e = value(k);
    switch (row(k).kind) {
        case KnobKind::Present: return e ? 1 : 0;
        case KnobKind::OffIfZero: return !(e && std::atoi(e) == 0) ? 1 : 0;
        case KnobKind::TriState: return !e ? -1 : std::atoi(e) != 0 ? 1 : 0;
        default: assert(!"knob_flag reads Present, OffIfZero and TriState knobs only"); return 0;
    }
}

int knob_clamped(Knob k, int hi) {
    const char* e = value(k);
    return e ? std::max(row(k).lo, std::min(hi, std::atoi(e))) : hi;
}

long long knob_count(Knob k, long long hi) {
    const char* e = value(k);
    if (!e) return -1;
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    return (end != e && *end == 0 && v >= 0 && v <= hi) ? v : -1;
}

double knob_seconds(Knob k) {
    const char* e = value(k);
    const double v = e ? std::atof(e) : 0.0;
    return v > 0.0 ? v : row(k).dflt;
}

}  // namespace pi
