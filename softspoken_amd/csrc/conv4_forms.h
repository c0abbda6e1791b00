// conv4.hip's launch forms, host side (no kernel in this header: tests/test_v4_forms.py compiles it alone).
// A form is one instantiation of conv3x3_v4_kernel: V4Form holds the kernel's template arguments.  It is described ONCE:
//   SS_V4_FORMS   the instantiated set.  conv4.hip expands it into the table {form, launch function}, this header into the bare forms:
//                 "is this form instantiated" is a lookup here, and a form that is not in the list is not launched, named or supported;
//   choose_v4     the only place where ConvArgs fields become form fields; it also decides the launch geometry.  What it states beside
//                 the kernel's own requirements is measured preference (which block takes which form); whether a form exists it asks the list;
//   v4_form_name  the instantiation's name as rocprofv3 prints it, from the form alone.
// launch_conv3x3_v4 (conv4.hip) is choose, look up, launch.
#pragma once
#include "kernels.h"
#include "mfma_util.h"
#include <algorithm>
#include <cstdio>

namespace ss {

static constexpr int kPixPitch = 80;     // LDS image of a patch, as conv2.hip
static constexpr int kRowPitch = 1664;
static constexpr int kPatch = 18;

struct V4Form { int NT, NW; bool BRES, RES, RADD, POOL; int RP; bool FIRST, FLAT, PF2, SPLIT, RANK1; int NH; bool GRES; };
constexpr bool operator==(const V4Form& a, const V4Form& b) {
    return a.NT == b.NT && a.NW == b.NW && a.BRES == b.BRES && a.RES == b.RES && a.RADD == b.RADD && a.POOL == b.POOL && a.RP == b.RP &&
           a.FIRST == b.FIRST && a.FLAT == b.FLAT && a.PF2 == b.PF2 && a.SPLIT == b.SPLIT && a.RANK1 == b.RANK1 && a.NH == b.NH && a.GRES == b.GRES;
}

// The instantiated forms.  Launch kinds: plain A (none of RES / RADD / RP), A with the r tensor (RES), B adding r (RADD, + POOL), B that
// computes the block's projection itself (RP K steps per stage, + POOL).
//    NT NW BRES RES RADD POOL RP FIRST FLAT PF2 SPLIT RANK1 NH GRES
#define SS_V4_FORMS(X)                                                                                                                \
    /* bf16, 4-wave tiles (8-row levels) */                                                                                           \
    X(1, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 4, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 4, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(1, 4, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 4, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0)                                              \
    X(2, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 4, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(2, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 4, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(2, 4, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 4, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0)                                              \
    X(3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 4, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(3, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 4, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(3, 4, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 4, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0)                                              \
    /* bf16, 8-wave tiles; PF2: the resident-bank launches of NT <= 2 but the NT = 2 A launch with r, which would spill */            \
    X(1, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 8, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(1, 8, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 8, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 8, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(1, 8, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0) X(1, 8, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0)                                              \
    X(1, 8, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0) X(1, 8, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0) X(1, 8, 1, 0, 1, 1, 0, 0, 0, 1, 0, 0, 1, 0)  \
    X(1, 8, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0)                                                                                          \
    X(2, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 8, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(2, 8, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 8, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 8, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(2, 8, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0) X(2, 8, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0)                                              \
    X(2, 8, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0) X(2, 8, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0) X(2, 8, 1, 0, 1, 1, 0, 0, 0, 1, 0, 0, 1, 0)  \
    X(3, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 8, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(3, 8, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 8, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 8, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0)  \
    X(3, 8, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0) X(3, 8, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0)                                              \
    /* bf16: conv1_1.B (FIRST), conv9_1.B (FLAT: adding r / four projection steps) */                                                 \
    X(1, 8, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0) X(1, 8, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0) X(1, 8, 1, 0, 0, 0, 4, 0, 1, 0, 0, 0, 1, 0)  \
    /* bf16, "projection in B", the blocks the network has: conv2_1, conv3_1, conv4_1, conv_bottleneck / encoder_out, and conv7: its A */ \
    /* launch gains more (473 -> 349 us) than B loses (165 -> 222); conv8 in that form: -46 / +144 us, no form built */               \
    X(2, 8, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0) X(3, 8, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 1, 0) X(2, 8, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 1, 0)  \
    X(1, 4, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 1, 0) X(2, 8, 1, 0, 0, 0, 6, 0, 0, 0, 0, 0, 1, 0)                                              \
    /* f16x2 (SPLIT), one tile per workgroup: NT = 1 (8- and 4-wave tiles) and NT = 3 (8-wave); no plain A launch */                  \
    X(1, 4, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0) X(1, 4, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0) X(1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0)  \
    X(1, 4, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0) X(1, 4, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0) X(1, 4, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0)  \
    X(1, 8, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0) X(1, 8, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0) X(1, 8, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0)  \
    X(1, 8, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0) X(1, 8, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0) X(1, 8, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0)  \
    X(3, 8, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0) X(3, 8, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0) X(3, 8, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0)  \
    X(3, 8, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0) X(3, 8, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0) X(3, 8, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0)  \
    /* f16x2: conv1_1.B (RANK1, with and without the first conv), conv9_1.B (FLAT), conv2_1.B with its projection */                  \
    X(1, 8, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0) X(1, 8, 1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0) X(1, 8, 1, 0, 1, 0, 0, 0, 1, 0, 1, 0, 1, 0)  \
    X(1, 8, 1, 0, 0, 0, 4, 0, 1, 0, 1, 0, 1, 0) X(1, 8, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 1, 0)                                              \
    /* f16x2, DUO: two 8-wave tiles over resident banks; four 4-wave tiles over the bank ring (BRES = 0) or resident banks (+ plain A) */ \
    X(1, 8, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 2, 0) X(1, 8, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 2, 0) X(1, 8, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 2, 0)  \
    X(1, 4, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 4, 0) X(1, 4, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 4, 0) X(1, 4, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 4, 0)  \
    X(1, 4, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 4, 0) X(1, 4, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 4, 0) X(1, 4, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 4, 0)  \
    X(1, 4, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 4, 0)                                                                                          \
    /* f16x2, GRES: one channel group per workgroup, its banks resident -- conv7.B, conv2_1.B (with its projection, or adding r) */    \
    X(1, 4, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 4, 1) X(1, 4, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 4, 1) X(1, 4, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 4, 1)

#define SS_V4_BARE(NT, NW, BRES, RES, RADD, POOL, RP, FIRST, FLAT, PF2, SPLIT, RANK1, NH, GRES) \
    V4Form{NT, NW, bool(BRES), bool(RES), bool(RADD), bool(POOL), RP, bool(FIRST), bool(FLAT), bool(PF2), bool(SPLIT), bool(RANK1), NH, bool(GRES)},
static constexpr V4Form kV4Forms[] = {SS_V4_FORMS(SS_V4_BARE)};
#undef SS_V4_BARE
static constexpr int kV4FormCount = (int)(sizeof kV4Forms / sizeof kV4Forms[0]);

// index of a form in the list (the same index in conv4.hip's launch table), -1: not instantiated
inline int v4_form_index(const V4Form& f) {
    for (int i = 0; i < kV4FormCount; ++i) if (kV4Forms[i] == f) return i;
    return -1;
}

// conv3x3_v4_kernel<NT, NW, BRES, RES, RADD, POOL, RP, FIRST, FLAT, PF2, SPLIT, RANK1, NH, GRES> as rocprofv3 prints it
inline const char* v4_form_name(const V4Form& f) {
    static thread_local char buf[160];
    auto tf = [](bool b) { return b ? "true" : "false"; };
    snprintf(buf, sizeof buf, "conv3x3_v4_kernel<%d, %d, %s, %s, %s, %s, %d, %s, %s, %s, %s, %s, %d, %s>", f.NT, f.NW, tf(f.BRES), tf(f.RES), tf(f.RADD),
             tf(f.POOL), f.RP, tf(f.FIRST), tf(f.FLAT), tf(f.PF2), tf(f.SPLIT), tf(f.RANK1), f.NH, tf(f.GRES));
    return buf;
}

// K steps of the projection a stage of a "projection in B" launch carries: ceil(steps / chunks), one of 1, 2, 4, 6
inline int v4_rp(const ConvArgs& a) {
    if (!a.proj_w) return 0;
    const int steps = (a.C0x + a.C1x) / 16, nch = (a.C0 + a.C1) / 32;
    const int per = (steps + nch - 1) / nch;
    return per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 6 ? 6 : -1;
}

#ifndef SS_RPROJ_DEFAULT
#define SS_RPROJ_DEFAULT 2
#endif
#ifndef SS_DUO_DEFAULT
#define SS_DUO_DEFAULT 4
#endif
#ifndef SS_GRES_DEFAULT
#define SS_GRES_DEFAULT 1
#endif
// a launch: the form (an entry of the list when ok) and its geometry; choose_v4 also writes a.tiles_y / a.tiles_x
struct V4Choice { bool ok; V4Form form; int grid, block, total, lds_b; size_t lds; };

inline V4Choice choose_v4(ConvArgs& a, int NT, int num_cus, int prec) {
    V4Choice c{};
    if (prec != 1 && prec != 2) return c;
    const bool split = prec == 2;
    if (!a.relu || a.R0 || a.R1) return c;
    const bool first = a.first_w != nullptr, flat = a.flat_part != nullptr, proj = a.proj_w != nullptr;
    const bool rank1 = split && a.rank1_src != nullptr;
    const int rp = v4_rp(a);
    if (split) {      // forms of the f16x2 mode: A with the r tensor, B adding it (+ pool, + flatten), conv1_1.B with the rank-1 residual
        if (a.lo_delta <= 0) return c;
        // "projection in B" (no r tensor): conv9_1.B (flatten form, four K steps on its one chunk) and conv2_1.B (two groups, pool, one
        // step per chunk); their A launches are `plain` and exist in the four-tile resident form only
        // (conv9_1 in this form: A 4020 -> 3440 us per 1005 windows, its flatten B launch 2375 -> 2740 us with the four steps in two
        // halves around part 1's loop -- with all eight fragments in flight at once it spilled 100 bytes and took 3640 us;
        // SOFTSPOKEN_RPROJ in the dev build: 0 = no block, 1 = conv2_1 only, 2 = conv2_1 and conv9_1)
        static const int rproj_env = dev_env("SOFTSPOKEN_RPROJ", SS_RPROJ_DEFAULT);
        if (proj && !(NT == 1 && a.H % 16 == 0 && ((flat && rp == 4 && rproj_env == 2) || (!flat && a.pool_out && a.Cout == 64 && rp == 1)))) return c;
        if (first && !rank1) return c;
        if (rank1 && !(NT == 1 && a.rank1_w && a.pool_out && !a.res_out && !a.res_in && !flat && a.C0 == 32 && a.C1 == 0 && a.H % 16 == 0)) return c;
    }
    if (flat && !(NT == 1 && a.Cout == 32 && a.C0 == 32 && a.C1 == 0 && a.H % 16 == 0 && a.flat_w4 && (a.res_in || rp == 4) && !a.pool_out && !first)) return c;
    if (first) {                                                                                  // conv1_1.B: features in, c1 + p1 out
        if (!(NT == 1 && a.Cout == 32 && a.C0 == 32 && a.C1 == 0 && a.H % 16 == 0 && a.first_b && a.rank1_src && a.rank1_w && a.pool_out &&
              !a.res_out && !a.res_in && !proj && !a.plain)) return c;
    } else if (proj) {                                                                            // B launch that computes the projection itself
        if (a.rank1_src || a.res_out || a.res_in || a.plain || rp < 0 || !a.xp0 || a.C0x % 16 || a.C1x % 16 || (a.C1x && !a.xp1)) return c;
        if (a.C0 != a.Cout || a.C1 != 0) return c;
        if ((double)a.N * a.H * a.W * std::max(a.C0x, a.C1x) * 2.0 + kHdr >= 4294967296.0) return c;
    } else if (a.plain) {                                                                         // A launch without the projection
        if (a.rank1_src || a.res_out || a.res_in || a.pool_out) return c;
    } else if (!rank1) {
        if (a.rank1_src) return c;
        if (!(a.res_out || a.res_in) || (a.res_out && (a.res_in || a.pool_out))) return c;        // A launch or B launch of a ResBlock
    }
    if (a.W % 16 != 0 || a.H % 8 != 0 || a.Cout % (32 * NT) != 0 || NT < 1 || NT > 3) return c;
    if (a.C0 % 32 || a.C1 % 32 || (a.C1 && ((a.H | a.W) & 1))) return c;
    if ((double)a.N * a.H * a.W * std::max(a.Cout, std::max(a.C0, a.C1)) * 2.0 + kHdr >= 4294967296.0) return c;   // 32-bit byte offsets
    const int nw = (a.H % 16 == 0) ? 8 : 4;
    const int th = 2 * nw;
    a.tiles_y = a.H / th; a.tiles_x = a.W / 16;
    const int ngroups = a.Cout / (32 * NT);
    const long total_l = (long)a.N * a.tiles_y * a.tiles_x * ngroups;
    if (total_l <= 0 || total_l > 0x7fffffff) return c;
    c.total = (int)total_l;
    const int tap_bytes = 2 * NT * 1024;
    const int taps = a.res_out ? 10 : 9;
    const int all_taps = ((a.C0 + a.C1) / 32) * taps;
    static const int bres_kb = dev_env("SOFTSPOKEN_BRES_KB", 72);
    const int banks = split ? 2 : 1;                                                              // f16x2: high and low halves of the weights
    const bool bres = ngroups == 1 && (size_t)all_taps * tap_bytes * banks <= (size_t)((first || flat || rank1) ? 72 : bres_kb) * 1024;
    c.lds_b = bres ? all_taps * tap_bytes * banks : taps * tap_bytes * banks;
    // bf16 "projection in B" over streamed banks: the NT = 3 form holds its ONE group's projection weights in LDS, the others read the
    // tile's group from memory and were built for several groups
    if (proj && !flat && !split && !bres && (NT == 3) != (ngroups == 1)) return c;
    // the ConvArgs fields as form fields, for a workgroup of nh tiles of nw_ waves
    auto form_of = [&](int nw_, bool bres_, int nh, bool gres) {
        const bool res = a.res_out != nullptr;
        return V4Form{NT, nw_, bres_, res, !res && !first && !a.plain && rp == 0 && !rank1, !res && a.pool_out != nullptr, rp, first, flat, false, split, rank1, nh, gres};
    };
    auto accept = [&](const V4Form& f, int grid, size_t lds) {
        c.form = f; c.grid = grid; c.block = 64 * f.NW * f.NH; c.lds = lds; c.ok = true;
        return c;
    };
    // DUO (conv3x3_v4_kernel): several tiles per 16-wave workgroup, a beat apart; one workgroup per CU.  2 x 8 waves or 4 x 4 waves
    // (SOFTSPOKEN_DUO in the dev build: 0, 2, 4)
    static const int duo_env = dev_env("SOFTSPOKEN_DUO", SS_DUO_DEFAULT);
    // (the four-tile form's tiles are 8 rows: it also takes the 8 x 16 level -- conv_bottleneck.A / encoder_out.A over the bank ring, one
    // whole picture per tile -- where the independent 4-wave blocks ran at 190 TFLOP/s)
    static const int duo8_env = dev_env("SOFTSPOKEN_DUO_H8", 1);
    // GRES: one channel group per workgroup, that group's banks resident (kernels.h: gres_item).  A B launch with several groups whose
    // ONE group's banks fit beside the patches: the 64 -> 64 blocks' (72 KB per group) -- conv7.B over four 8-row tiles, conv2_1.B
    // ("projection in B") likewise.  The other forms stage those 72 KB per (tile, group) or per quad.  conv2_1.B as two 16-row tiles with
    // the banks resident measured the same as the four 8-row tiles (tools/experiments/r06_conv2_1B_resident_two_tiles.patch).
    // (SOFTSPOKEN_GRES=0 in the dev build: the forms below, as before)
    static const int gres_env = dev_env("SOFTSPOKEN_GRES", SS_GRES_DEFAULT);
    if (gres_env && duo_env == 4 && split && ngroups > 1 && (nw == 8 || duo8_env)) {
        const int nh = 4, thd = 32 / nh;
        const V4Form f = form_of(16 / nh, true, nh, true);
        const size_t group_b = (size_t)all_taps * tap_bytes * banks;
        const size_t proj_b = proj ? (size_t)((a.C0x + a.C1x) / 16) * (a.Cout / 32) * 1024 * banks : 0;
        const size_t lds = nh * (size_t)(thd + 2) * kRowPitch + group_b + proj_b + (size_t)a.Cout * 4;
        const long total_pos = (long)a.N * (a.H / thd) * a.tiles_x;
        const int grid = total_pos <= 0x7fffffff / ngroups ? gres_grid(num_cus, (int)total_pos, ngroups, nh) : 0;
        if (v4_form_index(f) >= 0 && lds <= 160 * 1024 && gres_grid_ok(grid, ngroups)) {
            c.lds_b = (int)group_b;
            a.tiles_y = a.H / thd;
            c.total = (int)(total_pos * ngroups);
            return accept(f, grid, lds);
        }
    }
    if ((duo_env == 2 || duo_env == 4) && split && (nw == 8 || (duo_env == 4 && duo8_env))) {
        const int nh = duo_env, thd = 32 / nh;           // tile rows: 16 (8 waves) or 8 (4 waves)
        const size_t fixed = nh * (size_t)(thd + 2) * kRowPitch + (size_t)a.Cout * 4 * (a.res_out ? 2 : 1);
        const size_t chunk_b = (size_t)taps * tap_bytes * banks;
        const size_t all_b = (size_t)ngroups * all_taps * tap_bytes * banks;    // every channel group's banks (conv2_1.A: 2 x 40 KB)
        const bool bres_d = fixed + all_b <= 160 * 1024;
        static const int ring_env = dev_env("SOFTSPOKEN_RING", 1);
        // streamed banks: a two-slot ring shared by the four tiles.  A launches: conv7.A 1440 -> 1370 us, conv8.A 2040 -> 1960 us,
        // conv4_1.A 415 -> 390 us per 1005 windows.  B launches (residual loads, the long epilogue): the large ones lost 6-7 % in this
        // form in round 2; from the 32 x 64 level down it wins (round 3, same box: conv_bottleneck.B / encoder_out.B 186 -> 128 us,
        // conv4_1.B 515 -> 500, conv7.B 564 -> 556; the 96-channel blocks' B launches as three groups: conv3_1.B 1233 -> 1197, conv6.B 306 -> 289)
        const bool ring = !bres_d && nh == 4 && ring_env && (a.res_out != nullptr || ring_env == 2 || (a.H <= 32 && a.res_in != nullptr));
        const size_t lds = fixed + (bres_d ? all_b : 2 * chunk_b);
        const V4Form f = form_of(16 / nh, bres_d, nh, false);
        // measured (tools/ab_layers.sh, f16x2, 1005 windows, alternating runs on one box): with shared resident banks conv9_1.A
        // 4820 -> 4440 us as 2 x 8 waves and -> 4020 us as 4 x 4 waves (its 80 KB of banks fit beside the patches but not twice
        // beside one), conv8.B 650 -> 607 us (4 x 4); with streamed banks the 2 x 8 form lost 2-8 % (a half's bank commit sits in
        // the other half's multiply phase); conv9_1.B (FLAT) as 4 x 4: 2765 -> 2946 us, not taken (its epilogue is the long
        // phase, and the 8-row tiles read 11 % more halo)
        if ((bres_d || ring) && v4_form_index(f) >= 0 && lds <= 160 * 1024) {
            c.lds_b = (int)(bres_d ? all_b : chunk_b);
            a.tiles_y = a.H / thd;
            c.total = (int)((long)a.N * a.tiles_y * a.tiles_x * ngroups);
            int grid = (num_cus + 7) / 8 * 8;
            if (grid * nh > c.total) grid = ((c.total + nh - 1) / nh + 7) / 8 * 8;
            return accept(f, grid, lds);
        }
    }
    // one tile per workgroup
    const size_t lds = (size_t)(th + 2) * kRowPitch + c.lds_b + (size_t)a.Cout * 4 * (a.res_out ? 2 : 1) + (first ? (size_t)(32 + (th + 5) * 20) * 4 : 0) +
                       (flat ? (size_t)nw * 2 * 64 * 4 : 0) + (proj && (ngroups == 1 || split) ? (size_t)((a.C0x + a.C1x) / 16) * (split ? a.Cout / 32 : NT) * 1024 * banks : 0);
    V4Form f = form_of(nw, bres, 1, false);
    // PF2, two-stage prefetch: where the launch is LDS-limited to two blocks per CU anyway (resident weights) and NT <= 2 keeps it under
    // 128 registers -- and the form exists
    static const int pf2_env = dev_env("SOFTSPOKEN_PF2", 1);
    if (pf2_env && bres && !first && !flat && NT <= 2 && lds * 3 > 160 * 1024) {
        V4Form p = f;
        p.PF2 = true;
        if (v4_form_index(p) >= 0) f = p;
    }
    if (v4_form_index(f) < 0) return c;
    int bpc = (int)((160 * 1024) / lds);
    if (bpc < 1) return c;
    if (bpc > 3) bpc = 3;
    { static const int cap = dev_env("SOFTSPOKEN_BPC", 3); if (bpc > cap) bpc = cap; }      // (dev build: fewer blocks per CU)
    int grid = num_cus * bpc;
    if (grid > c.total) grid = c.total;
    grid = (grid + 7) / 8 * 8;
    return accept(f, grid, lds);
}

}  // namespace ss
