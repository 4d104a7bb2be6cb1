// rl_report.hpp — how a finished batch's requests are classified for the batch report
// (rl_tally_batch, rl_top_denied; kernels in rl_report.hip and rl_topk.hip, host side in
// rl_engine_query.cpp). Plain C++ with no HIP header, so tests/cpp/test_report_plan.cpp checks it
// on the CPU against a hand-written table; the kernels call the same functions.
//
// Request i of a batch is (limiter, op, permits) as submitted and (allowed, remaining) as
// answered; a NULL limiter array reads as limiter 0 and a NULL op array as RL_OP_ACQUIRE. With
// n_lim the engine's limiter count:
//  * Row: the limiter id if the engine knows it, else kTallyUnknown (255). RL_MAX_LIMITERS is
//    255, so known ids are 0..254 and row 255 is free for everything else.
//  * Class: the first rule that matches.
//      1. INVALID  limiter >= n_lim, or op > 2, or op == ACQUIRE and permits <= 0. This is the
//                  partition's own rule (rl_partition.hip), taken from the INPUTS: the answer
//                  cannot decide it, because a token bucket's remaining legitimately reads -2
//                  (RL_REMAINING_INVALID's value) after a time regression.
//      2. ERROR    allowed == 0 and remaining == RL_REMAINING_ERROR (-3).
//      3. PEEK / RESET by op.
//      4. ALLOWED  allowed != 0.
//      5. DENIED   otherwise. Those with remaining == RL_REMAINING_UNKNOWN (-1) are the token
//                  bucket's permits > maxPermits and are also counted as over_max.
//    One ambiguity is the ABI's own: a valid, denied token-bucket acquire whose balance reads
//    exactly -3 after a time regression is indistinguishable from rule 2 and counts as ERROR.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RL_REPORT_HD __host__ __device__
#else
#define RL_REPORT_HD
#endif

namespace rl {

constexpr uint32_t kTallyRows = 256;        // RL_TALLY_ROWS
constexpr uint32_t kTallyUnknown = 255;     // RL_TALLY_UNKNOWN
constexpr uint32_t kTallyWords = 12;        // u64 words of an rl_limiter_tally (the last two reserved)
constexpr int64_t kReportRemUnknown = -1;   // RL_REMAINING_UNKNOWN
constexpr int64_t kReportRemError = -3;     // RL_REMAINING_ERROR

enum ReportClass : uint32_t { kRcInvalid = 0, kRcError, kRcAllowed, kRcDenied, kRcPeek, kRcReset, kRcClasses };

// The counters of a row, in rl_limiter_tally's field order.
enum TallyCol : uint32_t { kTcRequests = 0, kTcInvalid, kTcErrors, kTcAllowed, kTcDenied, kTcOverMax,
                           kTcPeeks, kTcResets, kTcPermitsAllowed, kTcPermitsDenied, kTcCols };

RL_REPORT_HD inline uint32_t report_row(uint32_t limiter, uint32_t n_lim) {
    return limiter < n_lim ? limiter : kTallyUnknown;
}

RL_REPORT_HD inline uint32_t report_class(uint32_t limiter, uint32_t n_lim, uint32_t op, int32_t permits,
                                          uint8_t allowed, int64_t remaining) {
    if (limiter >= n_lim || op > 2u || (op == 0u && permits <= 0)) return kRcInvalid;
    if (allowed == 0 && remaining == kReportRemError) return kRcError;
    if (op == 1u) return kRcPeek;
    if (op == 2u) return kRcReset;
    return allowed != 0 ? kRcAllowed : kRcDenied;
}

RL_REPORT_HD inline bool report_over_max(uint32_t cls, int64_t remaining) {
    return cls == kRcDenied && remaining == kReportRemUnknown;
}

// The row counter a class is counted in (besides kTcRequests).
RL_REPORT_HD inline uint32_t report_class_col(uint32_t cls) {
    return cls == kRcInvalid ? kTcInvalid : cls == kRcError ? kTcErrors : cls == kRcAllowed ? kTcAllowed
         : cls == kRcDenied ? kTcDenied : cls == kRcPeek ? kTcPeeks : kTcResets;
}

}  // namespace rl
