// sr_s3_taps.h -- the x3 kernels' phase sets and the slot order of their tap fragments (sr_utd_s3.h: k_utd_s3;  sr_tail_s3.hip:
// k_tail_s3).  Pure constexpr functions and nothing of HIP, so a plain C++17 host compile accepts the file: tests/test_sr_blob_layout.py
// prints the table from it and compares it with the packers' order (sr_pack.py:_s3_slots).
//
// Tap algebra of (kernel 7, stride 3, padding 2): HR row 3m + r takes kernel row ky = r + 2 - 3 dy from LR row m + dy, columns alike.
// The nine phases (r, c) have 4 6 4 / 6 9 6 / 4 6 4 taps, 49 in all; wave wv owns the phase set
//     wave 0: (1,1) (0,0)  13 taps      wave 1: (0,1) (2,1)  12      wave 2: (1,0) (1,2)  12      wave 3: (0,2) (2,0) (2,2)  12
// and keeps its taps in slots 0 .. 12: phase by phase, dy then dx, each running +1, 0, -1 over its live offsets.
#pragma once

namespace {

constexpr int ph_cnt(int wv) { return wv == 3 ? 3 : 2; }
constexpr int ph_r(int wv, int p) { return wv == 0 ? (p == 0 ? 1 : 0) : wv == 2 ? 1 : (p == 0 ? 0 : 2); }
constexpr int ph_c(int wv, int p) { return wv == 0 ? (p == 0 ? 1 : 0) : wv == 1 ? 1 : wv == 2 ? (p == 0 ? 0 : 2) : (p == 1 ? 0 : 2); }
// phase x (a row or a column phase) and offset d in {+1, 0, -1}: kernel index x + 2 - 3 d, live when it lies in 0 .. 6
constexpr bool tap_ok(int x, int d) { return x + 2 - 3 * d >= 0 && x + 2 - 3 * d <= 6; }
constexpr int tap_cnt(int x) { return x == 1 ? 3 : 2; }
constexpr int tap_rank(int x, int d) { return 1 - d - (x == 0 ? 1 : 0); }   // position of d among the live offsets, +1 first
constexpr int ph_base(int wv, int p) {
    int s = 0;
    for (int i = 0; i < p; ++i) s += tap_cnt(ph_r(wv, i)) * tap_cnt(ph_c(wv, i));
    return s;
}
constexpr int tap_slot(int wv, int p, int dy, int dx) {
    return ph_base(wv, p) + tap_rank(ph_r(wv, p), dy) * tap_cnt(ph_c(wv, p)) + tap_rank(ph_c(wv, p), dx);
}
static_assert(ph_base(0, 2) == 13 && ph_base(1, 2) == 12 && ph_base(2, 2) == 12 && ph_base(3, 3) == 12, "tap counts of the phase sets");

}  // namespace
