// The extents of every stream step, checked without a device (tests/test_stream_extents.py builds this with
// -fsanitize=address,undefined and runs it).  Seeded populations of streams of every kind are driven through many steps of the
// host-only stages of softspoken_amd/csrc/stream_plan.h -- layout, the upload packer, commit -- with fake, distinct base addresses
// for the step's buffers and a seeded flags / averages "download".  After every layout, every range a descriptor reads or writes
// must lie inside the buffer it names at the size the layout demands (reads from the current arena halves and from the upload:
// inside a segment the last commit recorded / a piece the layout placed there), and the write ranges of one launch must not overlap.
#include "../softspoken_amd/csrc/stream_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>

using namespace ss;

namespace {

[[noreturn]] void die(const std::string& msg) {
    std::fprintf(stderr, "stream_extents: FAILED: %s\n", msg.c_str());
    std::exit(1);
}
#define REQUIRE(cond, what) do { if (!(cond)) die(std::string(what) + " (" #cond ")"); } while (0)

const char* kBufName[kStepBufs] = {"cur", "next", "up", "newlg", "avg", "flags", "fmap", "spec", "up3", "bout", "bprof", "raw_cur", "raw_next", "up2", "out", "outb"};
constexpr uintptr_t kSpan = (uintptr_t)1 << 40;           // buffer b is given the addresses [(b + 1) kSpan, (b + 2) kSpan)

std::map<std::string, int64_t> g_count;                   // descriptors checked, by kind
int64_t g_split_lanes = 0, g_shared_passes = 0, g_steps = 0, g_idle_before_push = 0, g_on_host_steps = 0;

typedef std::vector<std::pair<int64_t, int64_t>> Segs;    // byte ranges [lo, hi)

bool inside(const Segs& v, int64_t lo, int64_t hi) {
    for (const auto& s : v) if (lo >= s.first && hi <= s.second) return true;
    return false;
}

struct Checker {
    const StepBuffers& B;
    Segs cur, raw_cur, up;                                // what may be read in the current halves and in the upload
    struct W { int buf; int64_t lo, hi; };
    std::vector<W> writes;                                // of the launch being checked

    int locate(const void* p, int64_t& off, const char* what) const {
        const uintptr_t a = (uintptr_t)p;
        REQUIRE(a >= kSpan && a < (uintptr_t)(kStepBufs + 1) * kSpan, std::string(what) + ": an address outside every buffer");
        const int b = (int)(a / kSpan) - 1;
        off = (int64_t)(a - (uintptr_t)B.base[b]);
        return b;
    }
    void read(const void* p, int64_t bytes, const char* what) const {
        REQUIRE(bytes >= 0, std::string(what) + ": negative length");
        if (!bytes) return;
        int64_t lo;
        const int b = locate(p, lo, what);
        const std::string at = std::string(what) + ": read of " + kBufName[b] + " [" + std::to_string(lo) + ", " + std::to_string(lo + bytes) + ")";
        if (b == kCur) REQUIRE(inside(cur, lo, lo + bytes), at + " outside what the last commit recorded");
        else if (b == kRawCur) REQUIRE(inside(raw_cur, lo, lo + bytes), at + " outside what the last commit recorded");
        else if (b == kUp) REQUIRE(inside(up, lo, lo + bytes), at + " outside the pieces of the upload");
        else REQUIRE(lo + bytes <= (int64_t)B.need[b], at + " past need " + std::to_string(B.need[b]));
    }
    void write(const void* p, int64_t bytes, const char* what) {
        REQUIRE(bytes >= 0, std::string(what) + ": negative length");
        if (!bytes) return;
        int64_t lo;
        const int b = locate(p, lo, what);
        REQUIRE(b != kCur && b != kRawCur && b != kUp, std::string(what) + ": write to a buffer that is only read");
        REQUIRE(lo + bytes <= (int64_t)B.need[b], std::string(what) + ": write of " + kBufName[b] + " [" + std::to_string(lo) + ", " + std::to_string(lo + bytes) +
                                                   ") past need " + std::to_string(B.need[b]));
        writes.push_back(W{b, lo, lo + bytes});
    }
    void end_launch(const char* what) {
        std::sort(writes.begin(), writes.end(), [](const W& a, const W& b) { return a.buf != b.buf ? a.buf < b.buf : a.lo < b.lo; });
        for (size_t i = 1; i < writes.size(); ++i)
            REQUIRE(writes[i].buf != writes[i - 1].buf || writes[i].lo >= writes[i - 1].hi, std::string(what) + ": two writes of one launch overlap in " + kBufName[writes[i].buf]);
        writes.clear();
    }
};

// ---- what the last commit recorded -------------------------------------------------------------------------------------
void recorded_segments(const std::map<int, StreamRec>& all, size_t need_cur, size_t need_raw, Segs& cur, Segs& raw) {
    auto add = [&](Segs& to, int64_t lo, int64_t n, int64_t elem, size_t need, const char* what) {
        if (n <= 0) return;
        REQUIRE(lo >= 0 && (lo + n) * elem <= (int64_t)need, std::string("a record's ") + what + " segment lies past the half the last step built");
        to.emplace_back(lo * elem, (lo + n) * elem);
    };
    for (const auto& kv : all) {
        const StreamRec& s = kv.second;
        if (s.finished || s.on_host) continue;
        for (int l = 0; l < s.lanes; ++l) {
            add(cur, s.mono_off + l * s.mono_ls, s.mono_n, 4, need_cur, "mono");
            add(cur, s.sig_off + l * s.sig_ls, s.sig_n, 4, need_cur, "signal");
            add(cur, s.lg_off + l * s.lg_ls, s.lg_n * 256, 4, need_cur, "logits");
            if (s.bands_on && s.bs_ls) {
                const int64_t lane = s.bs_off + l * s.bs_ls;
                add(cur, lane, 2 * 256 * kBandAcc, 4, need_cur, "band accumulators");
                if (s.bs_n) {
                    REQUIRE(s.bs_n <= s.bs_stride && s.bs_sum_off + 2 * (255 * s.bs_stride + s.bs_n) <= s.bs_ls, "a record's carried sums leave their lane");
                    add(cur, lane + s.bs_sum_off, 2 * (255 * s.bs_stride + s.bs_n), 4, need_cur, "band sums");
                }
            }
        }
        if (s.out_on) add(raw, s.raw_off, (s.frames_in - s.frames_out) * s.frame_bytes(), 1, need_raw, "raw PCM");
    }
}

// ---- the step's descriptors ------------------------------------------------------------------------------------------------
void check_copies(Checker& ck, const std::vector<StreamCopy>& v, const char* what) {
    for (const StreamCopy& d : v) {
        if (d.src) ck.read(d.src, d.n * 4, what);
        ck.write(d.dst, d.n * 4, what);
        ++g_count[what];
    }
    ck.end_launch(what);
}

void check_step(Checker& ck, const std::vector<StreamRec*>& act, const StepBuild& b) {
    const StepBuffers& B = ck.B;
    check_copies(ck, b.pre, "StreamCopy pre");
    for (const StreamDecode& d : b.dec) {
        ck.read(B.at<unsigned char>(kUp, d.pcm_off), d.frames * d.channels * (int64_t)pcm_bytes_per_sample(d.format), "StreamDecode");
        ck.write(d.dst, d.frames * 4, "StreamDecode");
        ++g_count["StreamDecode"];
    }
    ck.end_launch("StreamDecode");
    for (const StreamDecodeChannels& d : b.decc) {
        REQUIRE(d.pcm_off % 16 == 0, "StreamDecodeChannels: pcm_off is no multiple of 16");
        ck.read(B.at<unsigned char>(kUp, d.pcm_off), d.frames * d.channels * (int64_t)pcm_bytes_per_sample(d.format), "StreamDecodeChannels");
        for (int c = 0; c < d.channels; ++c) ck.write(d.dst + c * d.stride, d.frames * 4, "StreamDecodeChannels");
        ++g_count["StreamDecodeChannels"];
    }
    ck.end_launch("StreamDecodeChannels");
    for (const StreamResample& r : b.res) {
        // the kernel's taps of outputs m0 .. m0 + n - 1: inputs floor(m M / L) - half + 1 .. floor(m M / L) + half, those inside [mono_base, frames)
        const int64_t lo = std::max(r.m0 * r.M / r.L - r.half + 1, r.mono_base), hi = std::min((r.m0 + r.n - 1) * r.M / r.L + r.half + 1, r.frames);
        if (hi > lo) ck.read(r.mono + (lo - r.mono_base), (hi - lo) * 4, "StreamResample");
        ck.write(r.out, r.n * 4, "StreamResample");
        ++g_count["StreamResample"];
    }
    ck.end_launch("StreamResample");
    // the passes: every window lies inside the signal its lane holds after the launches above, its logits inside the new-logits buffer
    REQUIRE((int64_t)b.winoff.size() == b.total_w && (size_t)b.total_w * 256 * 4 <= B.need[kNewlg], "window offsets and the new-logits buffer disagree");
    for (size_t k = 0; k < act.size(); ++k) {
        const StreamRec& s = *act[k];
        const StreamPlan& p = b.plans[k];
        const int64_t nw = p.i_end - s.win_run;
        for (int l = 0; l < s.lanes; ++l)
            for (int64_t i = 0; i < nw; ++i) {
                const int64_t off = b.winoff[(size_t)(p.w_at + l * nw + i)], lane = p.sig_off + l * p.sig_ls;
                REQUIRE(off >= lane && off + SS_WINDOW_SAMPLES <= lane + p.sig_len(), "window offset: a window leaves its lane's signal");
                REQUIRE((size_t)(lane + p.sig_len() + 64) * 4 <= B.need[kNext], "window offset: a lane's signal leaves the arena half");
                ++g_count["window offset"];
            }
    }
    // maps: the idle launch, then one launch per pass
    std::map<const void*, size_t> sum_owner;              // a lane's sums -> its stream
    for (size_t k = 0; k < act.size(); ++k)
        for (int l = 0; act[k]->bands_on && l < act[k]->lanes; ++l) sum_owner[B.at<double>(kNext, (b.plans[k].bs_off + l * b.plans[k].bs_ls) / 2 + 256 * kBandAcc)] = k;
    std::map<const void*, int> state;                     // a lane's sums: 0 not started, 1 started, 2 finished; entries counted apart
    std::map<const void*, int> entries;
    auto check_maps = [&](const std::vector<StreamMap>& v, int64_t slots, const char* what) {
        for (const StreamMap& m : v) {
            REQUIRE(m.n >= 0 && m.n <= m.stride && m.fin_n <= m.n, std::string(what) + ": bins and stride disagree");
            int& st = state[m.sum];
            REQUIRE(((m.flags & kMapInit) != 0) == (st == 0) && st != 2, std::string(what) + ": a lane's entries do not begin with kMapInit once");
            st = (m.flags & kMapFin) ? 2 : 1;
            ++entries[m.sum];
            if ((m.flags & kMapInit) && m.old_sum && m.old_n > 0) {
                REQUIRE(m.old_n <= m.old_stride, std::string(what) + ": carried bins and stride disagree");
                ck.read(m.old_sum, (255 * m.old_stride + m.old_n) * 8, what);
            }
            if (m.n > 0) ck.write(m.sum, (255 * m.stride + m.n) * 8, what);
            if ((m.flags & kMapFin) && m.fin_n > 0) ck.write(m.fmap, 256 * m.fin_n * 4, what);
            REQUIRE(m.i1 >= m.i0 && m.slot0 >= 0 && m.slot0 + (m.i1 - m.i0) <= slots, std::string(what) + ": spec slots past the pass");
            REQUIRE((size_t)slots * 65536 * 4 <= B.need[kSpec] || slots == 0, std::string(what) + ": the pass's spec output past the spec buffer");
            ++g_count["StreamMap"];
        }
        ck.end_launch(what);
    };
    check_maps(b.map_idle, 0, "StreamMap idle");
    for (int64_t q = 0; q < b.n_pass_band; ++q) {
        const int64_t i0 = b.total_w_plain + q * b.ch_band;
        check_maps(b.map_pass[(size_t)q], std::min<int64_t>(b.ch_band, b.total_w - i0), "StreamMap pass");
        std::map<size_t, int> owners;                     // streams with a lane in this pass
        for (const StreamMap& m : b.map_pass[(size_t)q]) ++owners[sum_owner.at(m.sum)];
        g_shared_passes += owners.size() >= 2;
    }
    for (const auto& kv : state) REQUIRE(kv.second == 2, "StreamMap: a lane's sums never reach kMapFin");
    REQUIRE((int64_t)state.size() == b.n_band_lanes, "StreamMap: not one set of entries per band lane");
    for (const auto& kv : entries) g_split_lanes += kv.second >= 2;
    check_copies(ck, b.post, "StreamCopy post");
    for (const StreamAvg& a : b.avg) {
        ck.read(a.logits, (a.W - a.w0) * 256 * 4, "StreamAvg");
        ck.write(B.at<double>(kAvg, a.out_off), a.nb * 8, "StreamAvg");
        ck.write(B.at<unsigned char>(kFlags, a.out_off), a.nb, "StreamAvg");
        ++g_count["StreamAvg"];
    }
    ck.end_launch("StreamAvg");
    for (const StreamUnion& u : b.uni) {
        ck.read(B.at<double>(kAvg, u.in_off), u.lanes * u.nb * 8, "StreamUnion");
        ck.read(B.at<unsigned char>(kFlags, u.in_off), u.lanes * u.nb, "StreamUnion");
        ck.write(B.at<double>(kAvg, u.out_off), u.nb * 8, "StreamUnion");
        ck.write(B.at<unsigned char>(kFlags, u.out_off), u.nb, "StreamUnion");
        ++g_count["StreamUnion"];
    }
    ck.end_launch("StreamUnion");
}

void check_bands(Checker& ck, const std::vector<StreamRec*>& act, const BandBuild& o) {
    const StepBuffers& B = ck.B;
    std::vector<const StreamRec*> owner;                  // of every descriptor
    for (const StreamRec* s : act) if (s->bands_on) for (int l = 0; l < s->lanes; ++l) owner.push_back(s);
    REQUIRE(owner.size() == o.bd.size(), "StreamBand: not one descriptor per band lane");
    for (size_t k = 0; k < o.bd.size(); ++k) {
        const StreamBand& d = o.bd[k];
        if (d.acc_old) ck.read(d.acc_old, kBandAcc * 256 * 8, "StreamBand");
        ck.write(d.acc, kBandAcc * 256 * 8, "StreamBand");
        ck.read(d.fmap, 256 * d.nb * 4, "StreamBand");
        REQUIRE(d.ev0 >= 0 && d.nev >= 0 && (size_t)(d.ev0 + d.nev) <= o.evs.size(), "StreamBand: events past the list");
        for (int e = d.ev0; e < d.ev0 + d.nev; ++e) {
            const StreamBandEv& ev = o.evs[(size_t)e];
            ++g_count["StreamBandEv"];
            if (ev.type != kEvEmitSnap && ev.type != kEvEmitPark) continue;
            REQUIRE(ev.rec >= 0 && ev.rec < (int64_t)owner[k]->r_out.size(), "StreamBandEv: a record the step did not return");
            const int64_t at = d.out0 + ev.rec * d.lanes + d.lane;
            ck.write(B.at<ss_region_band>(kBout, at), sizeof(ss_region_band), "StreamBand record");
            if (d.want_prof) ck.write(B.at<double>(kBprof, at * 256), 256 * 8, "StreamBand profile");
        }
        ++g_count["StreamBand"];
    }
    ck.end_launch("StreamBand");
}

void check_outputs(Checker& ck, const OutBuild& ob) {
    const StepBuffers& B = ck.B;
    const int64_t rng0 = output_ranges_off(ob.ops.size()), rng1 = rng0 + (int64_t)ob.rng_all.size() * 8;
    auto ranges = [&](const int64_t* p, int64_t n, const char* what) {
        const int64_t lo = (int64_t)((const unsigned char*)p - B.base[kUp2]);
        REQUIRE(lo >= rng0 && lo + n * 16 <= rng1 && rng1 <= (int64_t)B.need[kUp2], std::string(what) + ": ranges outside the range table");
    };
    for (const StreamSilence& d : ob.sil) {
        const int64_t fb = d.channels * (int64_t)pcm_bytes_per_sample(d.format);
        REQUIRE(d.n0 >= 0 && d.n0 <= d.n, "StreamSilence: n0");
        ck.read(d.seg0, d.n0 * fb, "StreamSilence");
        ck.read(d.seg1, (d.n - d.n0) * fb, "StreamSilence");
        ranges(d.ranges, d.n_ranges, "StreamSilence");
        ck.write(B.at<short>(kOut, d.out_off), d.n * d.channels * 2, "StreamSilence");
        ++g_count["StreamSilence"];
    }
    ck.end_launch("StreamSilence");
    for (const StreamSilenceSource& d : ob.srcs) {
        REQUIRE(d.n0 >= 0 && d.n0 <= d.n && d.out_off % 16 == 0, "StreamSilenceSource: n0 / out_off");
        ck.read(d.seg0, d.n0, "StreamSilenceSource");
        ck.read(d.seg1, d.n - d.n0, "StreamSilenceSource");
        ranges(d.ranges, d.n_ranges, "StreamSilenceSource");
        ck.write(B.at<unsigned char>(kOutb, d.out_off), d.n, "StreamSilenceSource");
        ++g_count["StreamSilenceSource"];
    }
    ck.end_launch("StreamSilenceSource");
    for (const StreamCopyBytes& d : ob.cpb) {
        ck.read(d.src, d.n, "StreamCopyBytes");
        ck.write(d.dst, d.n, "StreamCopyBytes");
        ++g_count["StreamCopyBytes"];
    }
    ck.end_launch("StreamCopyBytes");
}

// ---- the packer, on real memory of exactly the stated size (the sanitizer sees a write past it) ------------------------------
void pack_step(const StepBuild& b, size_t cap) {
    std::vector<unsigned char> mem(cap);
    UploadPacker pk(mem.data(), cap, (size_t)b.desc_off);
    for (const HostPiece& h : b.pieces) pk.piece(h);
    pk.put(b.pre); pk.put(b.post); pk.put(b.dec); pk.put(b.res); pk.put(b.avg); pk.put(b.winoff); pk.put(b.decc); pk.put(b.uni); pk.put(b.map_idle);
    for (const auto& v : b.map_pass) pk.put(v);
    REQUIRE(pk.ok && pk.at <= cap, "the step's upload does not fit the size the layout states");
}
void pack_bands(const BandBuild& o, size_t cap) {
    std::vector<unsigned char> mem(cap);
    UploadPacker pk(mem.data(), cap);
    pk.put(o.bd); pk.put(o.evs);
    REQUIRE(pk.ok, "the bands' upload does not fit the size the layout states");
}
void pack_outputs(const OutBuild& ob, size_t cap) {
    std::vector<unsigned char> mem(cap);
    UploadPacker pk(mem.data(), cap);
    const size_t n = ob.ops.size();
    pk.put(ob.sil.data(), ob.sil.size() * sizeof(StreamSilence), n * sizeof(StreamSilence));
    pk.put(ob.cpb.data(), ob.cpb.size() * sizeof(StreamCopyBytes), 2 * n * sizeof(StreamCopyBytes));
    pk.put(ob.srcs.data(), ob.srcs.size() * sizeof(StreamSilenceSource), n * sizeof(StreamSilenceSource));
    const size_t o_rng = pk.put(ob.rng_all);
    REQUIRE(pk.ok && o_rng == (size_t)output_ranges_off(n), "the output's upload does not fit the layout it was addressed by");
}

// ---- streams ------------------------------------------------------------------------------------------------------------
struct Kind { const char* name; int sr, ch, format; bool each, out_on, src_out, bands, prof; };
const Kind kKinds[] = {
    {"plain 16 kHz", 16000, 1, SS_PCM_S16, false, false, false, false, false},
    {"plain direct", 22050, 1, SS_PCM_S16, false, false, false, false, false},
    {"output mix 48 kHz", 48000, 2, SS_PCM_S16, false, true, false, false, false},
    {"each 48 kHz", 48000, 2, SS_PCM_S16, true, false, false, false, false},
    {"each direct x3 output", 22050, 3, SS_PCM_F32, true, true, false, false, false},
    {"bands mix 16 kHz", 16000, 1, SS_PCM_S16, false, false, false, true, false},
    {"bands mix 48 kHz output profiles", 48000, 2, SS_PCM_S16, false, true, false, true, true},
    {"bands each 48 kHz profiles", 48000, 2, SS_PCM_S16, true, false, false, true, true},
    {"bands each direct x3 output", 22050, 3, SS_PCM_S16, true, true, false, true, false},
    {"source mix 44.1 kHz 24 bit", 44100, 2, SS_PCM_S24, false, true, true, false, false},
    {"source each 8 kHz 8 bit", 8000, 2, SS_PCM_U8, true, true, true, false, false},
};
constexpr int kNumKinds = (int)(sizeof kKinds / sizeof kKinds[0]);

StreamRec open_stream(const Kind& k, std::mt19937_64& rng) {
    StreamRec s;
    s.format = k.format; s.sr = k.sr; s.ch = k.ch; s.thr = 0.1; s.mg.brk = (rng() % 3) * 0.25;
    s.step = SS_STEP_DEFAULT; s.per_step = step_samples(s.step);
    s.out_on = k.out_on; s.src_out = k.src_out;
    if (k.out_on) s.er = ss_stream_erase{0.05 * (double)(rng() % 3), 0.1 * (double)(rng() % 2)};
    s.bands_on = k.bands; s.want_prof = k.prof;
    s.set_lanes(k.each ? k.ch : 1);
    if (k.sr != SS_SAMPLE_RATE) {
        int a = k.sr, b = SS_SAMPLE_RATE;
        while (b) { const int t = a % b; a = b; b = t; }
        s.L = SS_SAMPLE_RATE / a; s.M = k.sr / a;
        s.half = (int)std::ceil(32.0 / std::min(1.0, (double)SS_SAMPLE_RATE / k.sr));
    }
    return s;
}

// the record ss_stream_import makes of the stream's image: the carried state in host vectors, the lanes back to back
void to_image_and_back(StreamRec& s) {
    if (s.on_host || s.finished) return;
    s.h_mono.assign((size_t)(s.lanes * s.mono_n), 0.f); s.h_sig.assign((size_t)(s.lanes * s.sig_n), 0.f); s.h_lg.assign((size_t)(s.lanes * s.lg_n * 256), 0.f);
    if (s.bands_on) s.h_band.assign((size_t)(s.lanes * 256 * (kBandAcc + s.bs_n)), 0.0);
    if (s.out_on) s.h_raw.assign((size_t)((s.frames_in - s.frames_out) * s.frame_bytes()), 0);
    s.mono_off = s.sig_off = s.lg_off = s.mono_ls = s.sig_ls = s.lg_ls = s.raw_off = 0;
    s.bs_off = s.bs_ls = s.bs_stride = s.bs_sum_off = 0;
    s.on_host = true;
}

struct Script { int first_push, close_gap, image_at; int64_t total, pushed = 0; bool one_frame; };

void run_population(uint64_t seed, int chunk, int n_streams) {
    std::mt19937_64 rng(seed);
    std::map<int, StreamRec> all;
    std::map<int, Script> script;
    for (int id = 0; id < n_streams; ++id) {
        const Kind& k = kKinds[id < kNumKinds ? id : (int)(rng() % kNumKinds)];
        all.emplace(id, open_stream(k, rng));
        Script sc{(int)(rng() % 5), (int)(rng() % 2), rng() % 2 ? (int)(3 + rng() % 6) : -1, (int64_t)(k.sr * (2.0 + (double)(rng() % 60) / 10.0)), 0, rng() % 4 == 0};
        if (rng() % 9 == 0) sc.total = 0;                 // closed with nothing pushed
        script.emplace(id, sc);
    }
    size_t need_cur = 0, need_raw = 0;
    for (int round = 0; round < 400; ++round) {
        bool any = false;
        for (auto& kv : all) {
            StreamRec& s = kv.second;
            Script& sc = script[kv.first];
            if (s.finished) continue;
            any = true;
            if (round == sc.image_at) to_image_and_back(s);
            if (s.closed || round < sc.first_push) continue;
            int64_t n = sc.one_frame && rng() % 3 == 0 ? 1 : (int64_t)(s.sr * (0.1 + (double)(rng() % 13) / 10.0));
            if (rng() % 7 == 0) n = 0;
            n = std::min(n, sc.total - sc.pushed);
            s.staged.insert(s.staged.end(), (size_t)(n * s.frame_bytes()), (unsigned char)(rng() & 0xff));
            s.staged_frames += n; sc.pushed += n;
            if (sc.pushed == sc.total && (sc.close_gap == 0 || n == 0)) s.closed = true;    // in the step of the last push, or a step later
        }
        if (!any) return;
        std::vector<StreamRec*> act;
        for (auto& kv : all) if (!kv.second.finished) act.push_back(&kv.second);
        for (const StreamRec* s : act) { g_idle_before_push += s->frames_in == 0 && s->staged_frames == 0 && !s->closed; g_on_host_steps += s->on_host; }
        // layout
        StepBuffers B;
        for (int k = 0; k < kStepBufs; ++k) B.base[k] = (unsigned char*)((uintptr_t)(k + 1) * kSpan);
        Checker ck{B, {}, {}, {}, {}};
        recorded_segments(all, need_cur, need_raw, ck.cur, ck.raw_cur);
        StepBuild b = plan_step(act, chunk, B);
        REQUIRE(build_step(b, act, B), "build_step: more descriptors than the stated maxima");
        for (int k = 0; k < kStepBufs; ++k) REQUIRE(B.need[k] < kSpan, "a buffer larger than the checker's address span");
        for (const HostPiece& h : b.pieces) {
            REQUIRE(h.off >= 0 && h.off + (int64_t)h.bytes <= b.desc_off, "a piece of the upload reaches into the descriptors");
            for (const auto& u : ck.up) REQUIRE(h.off >= u.second || h.off + (int64_t)h.bytes <= u.first || !h.bytes, "two pieces of the upload overlap");
            if (h.bytes) ck.up.emplace_back(h.off, h.off + (int64_t)h.bytes);
        }
        check_step(ck, act, b);
        pack_step(b, B.need[kUp]);
        // the "download": most bins covered, runs of bins above the threshold
        std::vector<double> h_avg((size_t)b.total_b);
        std::vector<unsigned char> h_flags((size_t)b.total_b);
        bool above = rng() % 2;
        for (size_t i = 0; i < h_flags.size(); ++i) {
            if (rng() % 40 == 0) above = !above;
            h_flags[i] = (unsigned char)((rng() % 50 ? 1 : 0) | (above ? 2 : 0));
            if (!(h_flags[i] & 1)) h_flags[i] = 0;
            h_avg[i] = (double)(rng() % 1000) / 1000.0;
        }
        commit_step(all, act, b, h_avg.data(), h_flags.data());
        need_cur = B.need[kNext];
        ++g_steps;
        if (b.n_band_lanes) {
            const BandBuild bb = layout_bands(act, b, B);
            check_bands(ck, act, bb);
            pack_bands(bb, B.need[kUp3]);
            std::vector<ss_region_band> rec((size_t)bb.n_rec);
            std::vector<double> prof((size_t)bb.n_rec * 256);
            commit_bands(act, rec.data(), prof.data());
        }
        OutBuild ob = plan_outputs(act, B);
        if (ob.ops.empty()) continue;
        build_outputs(ob, act, b, B);
        check_outputs(ck, ob);
        pack_outputs(ob, B.need[kUp2]);
        commit_outputs(act, ob);
        need_raw = B.need[kRawNext];
    }
    die("a population did not finish in 400 rounds");
}

}  // namespace

int main() {
    for (int chunk : {1, 4, 16})
        for (uint64_t seed = 1; seed <= 6; ++seed) run_population(seed * 7919 + (uint64_t)chunk, chunk, kNumKinds + 4);
    const char* kinds[] = {"StreamCopy pre", "StreamCopy post", "StreamDecode", "StreamDecodeChannels", "StreamResample", "StreamAvg", "StreamUnion", "StreamMap",
                           "window offset", "StreamSilence", "StreamSilenceSource", "StreamCopyBytes", "StreamBand", "StreamBandEv"};
    std::printf("stream_extents: %lld steps\n", (long long)g_steps);
    for (const char* k : kinds) {
        std::printf("  %-22s %lld\n", k, (long long)g_count[k]);
        if (!g_count[k]) die(std::string("no descriptor of kind ") + k + " was checked");
    }
    std::printf("  band lanes split over passes %lld, passes shared by lanes %lld, stream-steps before a first push %lld, stream-steps from an image %lld\n",
                (long long)g_split_lanes, (long long)g_shared_passes, (long long)g_idle_before_push, (long long)g_on_host_steps);
    if (!g_split_lanes) die("no band lane was split over at least two passes");
    if (!g_shared_passes || !g_idle_before_push || !g_on_host_steps) die("a case the populations must include did not occur");
    std::printf("stream_extents: ok\n");
    return 0;
}
