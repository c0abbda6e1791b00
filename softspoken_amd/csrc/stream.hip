// Streaming detection (include/softspoken.h, ss_stream_*): recordings whose PCM arrives in pieces, stepped together.  A step plans
// every stream on the host, uploads all staged pieces and its descriptors in one copy, and rebuilds the streams' carried state in the
// other half of a double-buffered arena:
//   copy (carried samples / logits, padding zeros) -> decode + mixdown -> resample -> windows (forward_chunk, passes across streams)
//   -> new logits behind the carried ones -> averaging of the bins that became final -> regions continued on the host.
// A stream opened in each-channel mode (ss_stream_open_channels, more than one channel) carries one lane per channel instead of the one
// mixdown lane: the lanes share the stream's plan and differ only in their arena segments; its pieces are decoded to one plane per
// channel, every lane goes through the copies, the resampler, the passes and the averaging with a descriptor of its own, and the bins
// that became final are merged (OR of the flags, fmax of the averages) into the series the host walks.
// Nothing of the stream state changes before the step has completed without SS_ERR_RANGE: the arena half the streams live in is only
// read, and the host records are updated at the end (commit), so a refused step leaves every stream as it was.
// Streams opened with output (ss_stream_open_output) then get their decided frames back as 16-bit PCM with the detected speech zeroed
// (plan_outputs / run_output / commit_outputs, behind the commit): the raw PCM not returned yet is carried in a byte arena of the same two-half discipline.
// Streams opened with bands (ss_stream_open_bands; include/softspoken.h "stream bands") return with every region its ss_region_band,
// bytes equal to ss_region_bands on the whole file: their windows run in passes of their own that store the spec head's output,
// stream_map_kernel adds each pass to float64 sums per non-final bin carried in the arena and turns the bins that became final into the
// float32 averaged maps, and -- behind the commit's region walk, whose decisions arrive as a short event list -- stream_band_kernel walks
// the final bins in order over one running accumulator and a snapshot per lane and evaluates the regions the walk returned.
#include "engine.h"
#include "bands.h"
#include "stream_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

namespace ss {

namespace {

// ---- bands: kernels (descriptors: stream_desc.h) ----
__device__ __forceinline__ int band_win_start(int i) { return (int)(((int64_t)512 * i + 5) / 10); }   // round(51.2 i), as sep_accumulate_kernel

// Thread = (bin t of the lane's step range, channel x band blockIdx.y), descriptor blockIdx.z.  A thread owns its sum through all the
// launches of a step, so start, addition and the final value follow one another in one thread.  The addition is
// sep_accumulate_kernel's arithmetic: the pass's windows over the bin are added to its float64 sum in ascending window order; passes and
// steps arrive in ascending window order too, so the sum is the whole-file one.  The final value is sep_finalize_kernel's: sum / count
// as float32, 0 for a bin no window covers (only behind the last window of a closed stream).  Loads of spec and stores of sums and
// maps run along the bins: consecutive threads, consecutive addresses.
__global__ __launch_bounds__(256) void stream_map_kernel(const StreamMap* __restrict__ ds, int nd, const float* __restrict__ spec) {
    const int cm = blockIdx.y;
    for (int k = blockIdx.z; k < nd; k += gridDim.z) {
        const StreamMap d = ds[k];
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < d.n; t += (int64_t)gridDim.x * 256) {
            const int64_t jb = d.b0 + t;
            const int j = (int)jb;
            double* sp = d.sum + (size_t)cm * d.stride + t;
            double s;
            if (d.flags & kMapInit) s = (d.old_sum && jb >= d.old_b0 && jb < d.old_b0 + d.old_n) ? d.old_sum[(size_t)cm * d.old_stride + (jb - d.old_b0)] : 0.0;
            else s = *sp;
            int lo = (int)((double)(j - 255) / 51.2) - 1;
            if (lo < 0) lo = 0;
            const int hi = (int)((double)j / 51.2) + 1;
            {
                const int a = lo < d.i0 ? (int)d.i0 : lo, b = hi > d.i1 - 1 ? (int)d.i1 - 1 : hi;
                for (int i = a; i <= b; ++i) {
                    const int dd = j - band_win_start(i);
                    if (dd < 0 || dd >= 256) continue;
                    s += (double)spec[((size_t)(d.slot0 + (i - d.i0)) * 256 + cm) * 256 + dd];
                }
            }
            *sp = s;
            if ((d.flags & kMapFin) && t < d.fin_n) {
                const int b = hi > d.i_end - 1 ? (int)d.i_end - 1 : hi;
                int n = 0;
                for (int i = lo; i <= b; ++i) {
                    const int dd = j - band_win_start(i);
                    n += dd >= 0 && dd < 256;
                }
                d.fmap[(size_t)cm * d.fin_n + t] = n ? (float)(s / (double)n) : 0.f;
            }
        }
    }
}

// Block = one band lane, thread = (spec channel, band).  The step's final bins are walked in ascending order: P(y) is added to the
// current tile's sum, and a tile is closed into the completed-tile sum behind every bin whose number ends a multiple of 64 -- a region's
// E is then completed tiles + current tile at its snapshot, term for term band_profile_kernel's tile sums added by band_bounds_kernel.
// The events are applied in the host's order (their positions never decrease); records and profiles leave by ordinary vector stores.
__global__ __launch_bounds__(256) void stream_band_kernel(const StreamBand* __restrict__ ds, const StreamBandEv* __restrict__ evs,
                                                          const double* __restrict__ hz, ss_region_band* __restrict__ out,
                                                          double* __restrict__ profile) {
#pragma clang fp contract(off)
    const StreamBand d = ds[blockIdx.x];
    const int t = threadIdx.x;
    double done = 0.0, cur = 0.0, sd = 0.0, sc = 0.0, pk = 0.0;
    if (d.acc_old) { done = d.acc_old[t]; cur = d.acc_old[256 + t]; sd = d.acc_old[512 + t]; sc = d.acc_old[768 + t]; pk = d.acc_old[1024 + t]; }
    int64_t j = d.b0;
    const int64_t end = d.b0 + d.nb;
    auto advance = [&](int64_t to) {
        if (to > end) to = end;
        for (; j < to; ++j) {
            cur += band_power(d.fmap[(size_t)t * d.nb + (j - d.b0)]);
            if ((j & 63) == 63) { done += cur; cur = 0.0; }
        }
    };
    for (int k = 0; k < d.nev; ++k) {
        const StreamBandEv ev = evs[d.ev0 + k];
        switch (ev.type) {
            case kEvReset: advance(ev.pos); done = 0.0; cur = 0.0; break;
            case kEvSnap: advance(ev.pos); sd = done; sc = cur; break;
            case kEvPark: pk = sd + sc; break;
            default: {
                const double e = ev.type == kEvEmitPark ? pk : sd + sc;
                const size_t o = (size_t)(d.out0 + ev.rec * d.lanes + d.lane);
                if (d.want_prof) profile[o * 256 + t] = e;
                band_bounds_block(e, ev.n_bins, d.speech_ch, d.q_low, d.q_high, hz, out + o);
            }
        }
    }
    advance(end);
    d.acc[t] = done; d.acc[256 + t] = cur; d.acc[512 + t] = sd; d.acc[768 + t] = sc; d.acc[1024 + t] = pk;
}

}  // namespace

// A buffer a step grows to what its layout demands and the set releases with itself: device memory (engine.h DevBuf: ensure's growth,
// 1.5x) or pinned host memory (need + need / 2, at least 64 KB).
struct PinBuf {
    unsigned char* p = nullptr; size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { if (p) hipHostFree(p); }
    int reserve(ss_ctx* c, size_t need) {
        if (need <= cap && p) return SS_OK;
        if (p) { HIPCHK(c, hipHostFree(p)); p = nullptr; cap = 0; }
        const size_t nc = std::max(need + need / 2, (size_t)1 << 16);
        HIPCHK(c, hipHostMalloc((void**)&p, nc, hipHostMallocDefault));
        cap = nc;
        return SS_OK;
    }
};

struct StreamSet {
    std::map<int, StreamRec> s;
    int next_id = 0;
    DevBuf<float> arena[2]; int cur = 0;
    DevBuf<unsigned char> d_up; PinBuf h_up;              // the step's upload: PCM, host carries, descriptors, window offsets
    DevBuf<float> d_newlg; DevBuf<double> d_avg; DevBuf<unsigned char> d_flags;
    std::vector<double> h_avg; std::vector<unsigned char> h_flags;
    // streams with output: the carried raw PCM in two halves like the arena, the step's second (small) upload of descriptors and
    // ranges, the step's output on the device and in pinned memory (d_outb / h_outb: the source-encoding streams', bytes)
    DevBuf<unsigned char> barena[2]; int bcur = 0;
    DevBuf<unsigned char> d_up2; PinBuf h_up2;
    DevBuf<short> d_out; PinBuf h_out;
    DevBuf<unsigned char> d_outb; PinBuf h_outb;
    // streams with bands: the step's final maps [bins][256] of every band lane, the upload of the walk's events and the lanes'
    // descriptors behind the flags download, the records and profiles on the device and in pinned memory, the 130 band edges, the
    // spec head's output of one pass of band windows
    DevBuf<float> d_fmap, d_spec;
    DevBuf<unsigned char> d_up3; PinBuf h_up3;
    DevBuf<ss_region_band> d_bout; DevBuf<double> d_bprof; PinBuf h_bres;
    DevBuf<double> d_hz;
};

void free_streams(ss_ctx* c) {
    delete c->streams;
    c->streams = nullptr;
}

}  // namespace ss

using namespace ss;

static StreamSet& streams_of(ss_ctx* c) {
    if (!c->streams) c->streams = new StreamSet();
    return *c->streams;
}

static StreamRec* find_stream(ss_ctx* c, int id) {
    if (!c || !c->streams) return nullptr;
    auto it = c->streams->s.find(id);
    return it == c->streams->s.end() ? nullptr : &it->second;
}

static int64_t state_bytes(const StreamRec& s) {
    return (int64_t)sizeof(StreamRec) + 4 * s.lanes * (s.mono_n + s.sig_n + s.lg_n * 256) + 8 * (int64_t)(3 * s.pk_run.size()) +
           (s.bands_on && !s.finished ? 8 * (int64_t)s.lanes * 256 * (kBandAcc + s.bs_n) : 0) +
           (s.out_on ? (s.frames_in - s.frames_out) * s.frame_bytes() + 8 * (int64_t)s.er_rng.size() : 0);
}

static int init_rates(ss_ctx* c, StreamRec& s) {
    if (s.sr == SS_SAMPLE_RATE) { s.L = s.M = 1; s.half = 0; s.d_taps = nullptr; return SS_OK; }
    return get_taps(c, s.sr, s.L, s.M, s.half, &s.d_taps);
}

static int open_stream(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase, bool out_on, int* id,
                       bool each = false, bool bands = false, const ss_band_params* bprm = nullptr, bool want_prof = false) {
    static const unsigned char one[8] = {0};
    int rc = check_pcm_args(c, one, format, sr, ch, 0);
    if (rc) return rc;
    // (a stream with output takes an infinite threshold: +inf is the plain transcode, -inf erases everything a window covers)
    if (!id || (out_on ? std::isnan(threshold) : !std::isfinite(threshold)) || !std::isfinite(break_s)) return fail(c, SS_ERR_ARG, "ss_stream_open: bad argument");
    if (!erase_ok(erase)) return fail(c, SS_ERR_ARG, "ss_stream_open_output: pad_s and min_len_s must be finite and >= 0");
    if (bands) {
        std::string err;
        if (check_band_args(nullptr, 0, bprm, err)) return fail(c, SS_ERR_ARG, "ss_stream_open_bands: " + err);
    }
    if (!c->has_model) return fail(c, SS_ERR_STATE, "context was created without weights (audio-only)");
    if (bands && c->step != SS_STEP_DEFAULT)
        return fail(c, SS_ERR_STATE, "ss_stream_open_bands: bands need the default window step (the maps are defined on 0.6 s windows)");
    hipSetDevice(c->device);
    StreamRec s;
    s.bands_on = bands; s.want_prof = bands && want_prof; if (bands && bprm) s.bprm = *bprm;
    s.format = format; s.sr = sr; s.ch = ch; s.thr = threshold; s.mg.brk = break_s;
    s.step = c->step; s.per_step = step_samples(c->step);
    s.out_on = out_on; if (erase) s.er = *erase;
    s.set_lanes(each ? ch : 1);                          // (one channel in each-channel mode: a plain stream)
    if ((rc = init_rates(c, s))) return rc;
    StreamSet& S = streams_of(c);
    *id = S.next_id++;
    S.s.emplace(*id, std::move(s));
    return SS_OK;
}

extern "C" int ss_stream_open(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, int* id) {
    return open_stream(c, format, sr, ch, threshold, break_s, nullptr, false, id);
}

extern "C" int ss_stream_open_output(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase,
                                     int* id) {
    return open_stream(c, format, sr, ch, threshold, break_s, erase, true, id);
}

extern "C" int ss_stream_open_channels(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase,
                                       int with_output, int* id) {
    return open_stream(c, format, sr, ch, threshold, break_s, erase, erase != nullptr || with_output != 0, id, true);
}

// a stream with output in its own encoding: ss_stream_open_channels' stream (each_channel == 0: the mix's) read through
// ss_stream_output_bytes
extern "C" int ss_stream_open_source(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase,
                                     int each_channel, int* id) {
    int rc = open_stream(c, format, sr, ch, threshold, break_s, erase, true, id, each_channel != 0);
    if (rc) return rc;
    find_stream(c, *id)->src_out = true;
    return SS_OK;
}

extern "C" int ss_stream_open_bands(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase,
                                    int with_output, int each_channel, const ss_band_params* params, int want_profile, int* id) {
    return open_stream(c, format, sr, ch, threshold, break_s, erase, erase != nullptr || with_output != 0, id, each_channel != 0, true, params,
                       want_profile != 0);
}

extern "C" int ss_stream_push(ss_ctx* c, int id, const void* pcm, int64_t frames) {
    StreamRec* s = find_stream(c, id);
    if (!s) return fail(c, SS_ERR_ARG, "ss_stream_push: no such stream");
    if (s->closed) return fail(c, SS_ERR_STATE, "ss_stream_push: the stream is closed");
    int rc = check_pcm_args(c, pcm, s->format, s->sr, s->ch, frames);
    if (rc) return rc;
    if (s->frames_in + s->staged_frames + frames > ((int64_t)1 << 36)) return fail(c, SS_ERR_ARG, "ss_stream_push: stream too long");
    const size_t nb = (size_t)frames * s->ch * pcm_bytes_per_sample(s->format);
    if (nb) s->staged.insert(s->staged.end(), (const unsigned char*)pcm, (const unsigned char*)pcm + nb);
    s->staged_frames += frames;
    return SS_OK;
}

extern "C" int ss_stream_close(ss_ctx* c, int id) {
    StreamRec* s = find_stream(c, id);
    if (!s) return fail(c, SS_ERR_ARG, "ss_stream_close: no such stream");
    s->closed = true;
    return SS_OK;
}

extern "C" int ss_stream_free(ss_ctx* c, int id) {
    if (!find_stream(c, id)) return fail(c, SS_ERR_ARG, "ss_stream_free: no such stream");
    c->streams->s.erase(id);
    return SS_OK;
}

extern "C" int ss_stream_get_info(ss_ctx* c, int id, ss_stream_info* out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !out) return fail(c, SS_ERR_ARG, "ss_stream_get_info: bad argument");
    memset(out, 0, sizeof(*out));
    out->frames_pushed = s->frames_in + s->staged_frames;
    out->frames_staged = s->staged_frames;
    out->windows_run = s->win_run;
    out->windows_ready = s->finished ? 0 : plan_stream(*s).i_end - s->win_run;
    out->final_until_s = (double)s->bins_done * 3.0 / 256.0 - 3.0;
    out->closed = s->closed; out->finished = s->finished;
    out->state_bytes = state_bytes(*s);
    return SS_OK;
}

extern "C" int ss_stream_regions(ss_ctx* c, int id, ss_region* out, int64_t cap, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_regions: bad argument");
    *n_out = (int64_t)s->r_out.size();
    if (!out) return SS_OK;
    if (cap < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_regions: capacity < " + std::to_string(*n_out));
    if (*n_out) memcpy(out, s->r_out.data(), s->r_out.size() * sizeof(ss_region));
    return SS_OK;
}

extern "C" int ss_stream_avg(ss_ctx* c, int id, double* avg, int64_t* bin_idx, int64_t cap, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_avg: bad argument");
    *n_out = (int64_t)s->a_out.size();
    if (!avg && !bin_idx) return SS_OK;
    if (cap < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_avg: capacity < " + std::to_string(*n_out));
    if (*n_out && avg) memcpy(avg, s->a_out.data(), s->a_out.size() * 8);
    if (*n_out && bin_idx) memcpy(bin_idx, s->b_out.data(), s->b_out.size() * 8);
    return SS_OK;
}

extern "C" int ss_stream_avg_channel(ss_ctx* c, int id, int channel, double* avg, int64_t* bin_idx, int64_t cap, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_avg_channel: bad argument");
    if (channel < 0 || channel >= s->lanes) return fail(c, SS_ERR_ARG, "ss_stream_avg_channel: no such channel (a mix stream has channel 0 only)");
    if (s->lanes == 1) return ss_stream_avg(c, id, avg, bin_idx, cap, n_out);
    *n_out = (int64_t)s->b_out.size();
    if (!avg && !bin_idx) return SS_OK;
    if (cap < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_avg_channel: capacity < " + std::to_string(*n_out));
    if (*n_out && avg) memcpy(avg, s->la_out.data() + (size_t)channel * s->b_out.size(), s->b_out.size() * 8);
    if (*n_out && bin_idx) memcpy(bin_idx, s->b_out.data(), s->b_out.size() * 8);
    return SS_OK;
}

extern "C" int ss_stream_region_peaks(ss_ctx* c, int id, double* peaks, int64_t cap_regions, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_region_peaks: bad argument");
    if (s->lanes == 1) return fail(c, SS_ERR_STATE, "ss_stream_region_peaks: not an each-channel stream of several channels (ss_stream_open_channels)");
    *n_out = (int64_t)s->r_out.size();
    if (!peaks) return SS_OK;
    if (cap_regions < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_region_peaks: capacity < " + std::to_string(*n_out) + " regions");
    if (!s->p_out.empty()) memcpy(peaks, s->p_out.data(), s->p_out.size() * 8);
    return SS_OK;
}

extern "C" int ss_stream_bands(ss_ctx* c, int id, ss_region_band* out, double* profile, int64_t cap_regions, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_bands: bad argument");
    if (!s->bands_on) return fail(c, SS_ERR_STATE, "ss_stream_bands: the stream was opened without bands (ss_stream_open_bands)");
    if (profile && !s->want_prof) return fail(c, SS_ERR_STATE, "ss_stream_bands: the stream was opened without want_profile");
    *n_out = (int64_t)s->r_out.size();
    if (!out && !profile) return SS_OK;
    if (cap_regions < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_bands: capacity < " + std::to_string(*n_out) + " regions");
    if (out && !s->bd_out.empty()) memcpy(out, s->bd_out.data(), s->bd_out.size() * sizeof(ss_region_band));
    if (profile && !s->bp_out.empty()) memcpy(profile, s->bp_out.data(), s->bp_out.size() * 8);
    return SS_OK;
}

extern "C" int ss_stream_output(ss_ctx* c, int id, int16_t* out, int64_t cap_frames, int64_t* first_frame, int64_t* n_frames) {
    StreamRec* s = find_stream(c, id);
    if (!s || !first_frame || !n_frames) return fail(c, SS_ERR_ARG, "ss_stream_output: bad argument");
    if (!s->out_on) return fail(c, SS_ERR_STATE, "ss_stream_output: the stream was opened without output (ss_stream_open_output)");
    if (s->src_out) return fail(c, SS_ERR_STATE, "ss_stream_output: the stream's output is in its own encoding (ss_stream_output_bytes)");
    *first_frame = s->o_first; *n_frames = s->o_n;
    if (!out) return SS_OK;
    if (cap_frames < s->o_n) return fail(c, SS_ERR_CAPACITY, "ss_stream_output: capacity < " + std::to_string(s->o_n));
    if (s->o_n) memcpy(out, (const int16_t*)c->streams->h_out.p + s->o_off, (size_t)(s->o_n * s->ch) * 2);
    return SS_OK;
}

extern "C" int ss_stream_output_bytes(ss_ctx* c, int id, void* out, int64_t cap_bytes, int64_t* first_frame, int64_t* n_frames) {
    StreamRec* s = find_stream(c, id);
    if (!s || !first_frame || !n_frames) return fail(c, SS_ERR_ARG, "ss_stream_output_bytes: bad argument");
    if (!s->src_out) return fail(c, SS_ERR_STATE, "ss_stream_output_bytes: the stream was not opened with ss_stream_open_source");
    *first_frame = s->o_first; *n_frames = s->o_n;
    if (!out) return SS_OK;
    const int64_t bytes = s->o_n * s->frame_bytes();
    if (cap_bytes < bytes) return fail(c, SS_ERR_CAPACITY, "ss_stream_output_bytes: capacity < " + std::to_string(bytes));
    if (bytes) memcpy(out, c->streams->h_outb.p + s->o_off, (size_t)bytes);
    return SS_OK;
}

extern "C" int ss_stream_get_output_info(ss_ctx* c, int id, ss_stream_output_info* out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !out) return fail(c, SS_ERR_ARG, "ss_stream_get_output_info: bad argument");
    if (!s->out_on) return fail(c, SS_ERR_STATE, "ss_stream_get_output_info: the stream was opened without output (ss_stream_open_output)");
    memset(out, 0, sizeof(*out));
    out->frames_out = s->frames_out; out->frames_held = s->frames_in + s->staged_frames - s->frames_out; out->frames_erased = s->erased;
    out->pad_s = s->er.pad_s; out->min_len_s = s->er.min_len_s;
    return SS_OK;
}

// ------------------------------------------------------------------------------------------------------
// the step: layout (stream_plan.h, host only) -> run (below: grow, pack, upload, launch, download) -> commit (stream_plan.h), then the
// same three for the bands and for the output, which are planned from the committed records
// ------------------------------------------------------------------------------------------------------
// a device buffer of the step at the size the layout states (0: the step does not use it), and its base for the descriptors
template <typename T>
static int grow(ss_ctx* c, DevBuf<T>& buf, StepBuffers& B, StepBuf which) {
    if (B.need[which]) { int rc = buf.reserve_bytes(c, B.need[which]); if (rc) return rc; }
    B.base[which] = (unsigned char*)buf.p;
    return SS_OK;
}

// the packed upload to the device, after the packer has taken everything: `bytes` of it
static int upload(ss_ctx* c, const UploadPacker& pk, unsigned char* dst, size_t bytes, const char* what) {
    if (!pk.ok) return fail(c, SS_ERR_STATE, std::string("ss_stream_step: the ") + what + " upload does not fit its layout");
    HIPCHK(c, hipMemcpyAsync(dst, pk.base, bytes, hipMemcpyHostToDevice, c->stream));
    return SS_OK;
}

static int launch_maps(ss_ctx* c, const unsigned char* d_up, size_t off, size_t n, int64_t max_n, const float* spec, double bytes) {
    if (!n) return SS_OK;
    ScopedLaunch sl(c, c->stream, "stream_map_kernel", 0.0, bytes);
    hipLaunchKernelGGL(stream_map_kernel, dim3((unsigned)std::min<int64_t>((max_n + 255) / 256, 64), 256, (unsigned)std::min<size_t>(n, 4096)), dim3(256), 0,
                       c->stream, (const StreamMap*)(d_up + off), (int)n, spec);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

// where the packer put the step's descriptor vectors
struct StepOffsets { size_t pre, post, dec, res, avg, win, decc, uni, midle; std::vector<size_t> mpass; };

static int run_upload(ss_ctx* c, StreamSet& S, const StepBuild& b, const StepBuffers& B, StepOffsets& o) {
    UploadPacker pk(S.h_up.p, B.need[kUp], (size_t)b.desc_off);    // (the stated size: what the device buffer is sure to hold)
    for (const HostPiece& h : b.pieces) pk.piece(h);
    o.pre = pk.put(b.pre); o.post = pk.put(b.post); o.dec = pk.put(b.dec); o.res = pk.put(b.res); o.avg = pk.put(b.avg); o.win = pk.put(b.winoff);
    o.decc = pk.put(b.decc);                                   // (nothing, and no bytes, without an each-channel stream)
    o.uni = pk.put(b.uni);
    o.midle = pk.put(b.map_idle);
    for (const auto& v : b.map_pass) o.mpass.push_back(pk.put(v));
    return upload(c, pk, S.d_up.p, pk.at, "step's");
}

// copies, decode, resample in front of the passes
static int run_front(ss_ctx* c, StreamSet& S, const StepBuild& b, const StepOffsets& o) {
    const unsigned char* up = S.d_up.p;
    {
        ScopedLaunch sl(c, c->stream, "stream_copy", 0.0, 8.0 * b.max_copy * b.pre.size());
        HIPCHK(c, launch_stream_copy((const StreamCopy*)(up + o.pre), (int)b.pre.size(), b.max_copy, c->stream));
    }
    {
        ScopedLaunch sl(c, c->stream, "stream_decode", 0.0, 0.0);
        HIPCHK(c, launch_stream_decode(up, (const StreamDecode*)(up + o.dec), (int)b.dec.size(), b.max_dec, c->stream));
    }
    if (!b.decc.empty()) {
        ScopedLaunch sl(c, c->stream, "stream_decode_channels", 0.0, b.decc_bytes);
        HIPCHK(c, launch_stream_decode_channels(up, (const StreamDecodeChannels*)(up + o.decc), (int)b.decc.size(), b.max_decc, c->stream));
    }
    {
        ScopedLaunch sl(c, c->stream, "stream_resample", 0.0, 0.0);
        HIPCHK(c, launch_stream_resample((const StreamResample*)(up + o.res), (int)b.res.size(), b.max_res, c->stream));
    }
    return SS_OK;
}

// the windows: the plain streams' passes, then the band streams', each followed by its map launch
static int run_passes(ss_ctx* c, StreamSet& S, const StepBuild& b, const StepOffsets& o) {
    int rc;
    const float* A = S.arena[S.cur ^ 1].p;
    const int64_t* d_win = (const int64_t*)(S.d_up.p + o.win);
    if (b.total_w > 0) {
        if ((rc = ensure_workspace(c, std::max(b.total_w_plain > 0 ? b.ch_plain : 1, b.total_w_band > 0 ? b.ch_band : 1)))) return rc;
        for (int64_t i0 = 0; i0 < b.total_w_plain; i0 += b.ch_plain) {
            const int m = (int)std::min<int64_t>(b.ch_plain, b.total_w_plain - i0);
            if ((rc = forward_chunk(c, c->ws[0], c->stream, A, d_win + i0, m, S.d_newlg.p + (size_t)i0 * 256, nullptr))) return rc;
        }
    }
    if (!b.n_band_lanes) return SS_OK;
    // a lane's first entry starts its sums from the carried ones, every pass of its windows adds that pass's spec output, its last
    // entry turns the final bins into maps (lanes without a window: one entry of their own, before the passes)
    if ((rc = launch_maps(c, S.d_up.p, o.midle, b.map_idle.size(), b.max_map_n, nullptr, 16.0 * 256 * b.max_map_n * b.map_idle.size()))) return rc;
    for (int64_t q = 0; q < b.n_pass_band; ++q) {
        const int64_t i0 = b.total_w_plain + q * b.ch_band;
        const int m = (int)std::min<int64_t>(b.ch_band, b.total_w - i0);
        const size_t n = b.map_pass[(size_t)q].size();
        if ((rc = forward_chunk(c, c->ws[0], c->stream, A, d_win + i0, m, S.d_newlg.p + (size_t)i0 * 256, S.d_spec.p))) return rc;
        if ((rc = launch_maps(c, S.d_up.p, o.mpass[(size_t)q], n, b.max_map_n, S.d_spec.p, (double)m * 2 * 32768 * 4 + 16.0 * 256 * b.max_map_n * n))) return rc;
    }
    return SS_OK;
}

// new logits behind the carried ones, averaging, the merge of the lanes, the download
static int run_back(ss_ctx* c, StreamSet& S, const StepBuild& b, const StepOffsets& o) {
    const unsigned char* up = S.d_up.p;
    {
        int64_t mx = 0; for (const StreamCopy& p : b.post) mx = std::max(mx, p.n);
        ScopedLaunch sl(c, c->stream, "stream_copy", 0.0, 8.0 * mx * b.post.size());
        HIPCHK(c, launch_stream_copy((const StreamCopy*)(up + o.post), (int)b.post.size(), mx, c->stream));
    }
    {
        ScopedLaunch sl(c, c->stream, "stream_average", 0.0, b.avg_reads * 4 + (double)b.total_b * 9);
        HIPCHK(c, launch_stream_average((const StreamAvg*)(up + o.avg), (int)b.avg.size(), b.max_bins, S.d_avg.p, S.d_flags.p, c->stream));
    }
    if (!b.uni.empty()) {
        ScopedLaunch sl(c, c->stream, "stream_union", 0.0, b.uni_bytes);
        HIPCHK(c, launch_stream_union((const StreamUnion*)(up + o.uni), (int)b.uni.size(), b.max_uni, S.d_avg.p, S.d_flags.p, c->stream));
    }
    S.h_avg.resize((size_t)b.total_b); S.h_flags.resize((size_t)b.total_b);
    if (b.total_b) {
        HIPCHK(c, hipMemcpyAsync(S.h_avg.data(), S.d_avg.p, (size_t)b.total_b * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.h_flags.data(), S.d_flags.p, (size_t)b.total_b, hipMemcpyDeviceToHost, c->stream));
    }
    return SS_OK;
}

// The step's device work.  Nothing of a record is changed here: a refused step (SS_ERR_RANGE) leaves every stream as it was.
static int run_step(ss_ctx* c, StreamSet& S, const std::vector<StreamRec*>& act, StepBuild& b, StepBuffers& B) {
    int rc;
    const int nxt = S.cur ^ 1;
    B.base[kCur] = (unsigned char*)S.arena[S.cur].p;
    if ((rc = grow(c, S.arena[nxt], B, kNext)) || (rc = grow(c, S.d_up, B, kUp)) || (rc = S.h_up.reserve(c, B.need[kUp])) || (rc = grow(c, S.d_newlg, B, kNewlg)) ||
        (rc = grow(c, S.d_avg, B, kAvg)) || (rc = grow(c, S.d_flags, B, kFlags)) || (rc = grow(c, S.d_fmap, B, kFmap)) || (rc = grow(c, S.d_spec, B, kSpec)))
        return rc;
    if (!build_step(b, act, B)) return fail(c, SS_ERR_STATE, "ss_stream_step: more descriptors than the upload was sized for");
    StepOffsets o;
    if ((rc = run_upload(c, S, b, B, o)) || (rc = run_front(c, S, b, o)) || (rc = range_clear(c, c->stream)) || (rc = run_passes(c, S, b, o)) ||
        (rc = run_back(c, S, b, o)) || (rc = range_fetch(c, c->stream)))
        return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    if (range_left(c))
        return fail(c, SS_ERR_RANGE, "f16x2: an activation left the f16 range (|x| > 65504) or was not finite; nothing of the step is committed: "
                                     "move the streams that had windows in it to an fp32 context (ss_stream_export / ss_stream_import)");
    return SS_OK;
}

// one launch walks every band lane, one copy brings the records (and profiles) to pinned memory
static int run_bands(ss_ctx* c, StreamSet& S, const BandBuild& o, StepBuffers& B) {
    int rc;
    if ((rc = grow(c, S.d_up3, B, kUp3)) || (rc = S.h_up3.reserve(c, B.need[kUp3])) || (rc = grow(c, S.d_bout, B, kBout)) || (rc = grow(c, S.d_bprof, B, kBprof)) ||
        (rc = S.h_bres.reserve(c, o.rec_bytes + o.prof_bytes + 64)))
        return rc;
    if (!S.d_hz.p) {
        double f[130];
        band_edges(f);
        if ((rc = S.d_hz.reserve(c, 130))) return rc;
        HIPCHK(c, hipMemcpy(S.d_hz.p, f, sizeof f, hipMemcpyHostToDevice));
    }
    UploadPacker pk(S.h_up3.p, B.need[kUp3]);
    pk.put(o.bd);
    const size_t o_ev = pk.put(o.evs);
    if ((rc = upload(c, pk, S.d_up3.p, pk.used, "bands'"))) return rc;
    {
        ScopedLaunch sl(c, c->stream, "stream_band_kernel", 0.0, o.bins * 1024 + (double)o.bd.size() * kBandAcc * 4096 + (double)o.n_rec * (48 + (o.any_prof ? 2048 : 0)));
        hipLaunchKernelGGL(stream_band_kernel, dim3((unsigned)o.bd.size()), dim3(256), 0, c->stream, (const StreamBand*)S.d_up3.p, (const StreamBandEv*)(S.d_up3.p + o_ev),
                           S.d_hz.p, S.d_bout.p, S.d_bprof.p);
        HIPCHK(c, hipGetLastError());
    }
    if (o.n_rec) {
        HIPCHK(c, hipMemcpyAsync(S.h_bres.p, S.d_bout.p, (size_t)o.n_rec * sizeof(ss_region_band), hipMemcpyDeviceToHost, c->stream));
        if (o.any_prof) HIPCHK(c, hipMemcpyAsync(S.h_bres.p + o.rec_bytes, S.d_bprof.p, o.prof_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    return SS_OK;
}

// one launch encodes every stream's decided frames (one more those in the streams' own encoding), one copies the raw PCM that stays,
// one copy (each) brings the output to pinned memory
static int run_output(ss_ctx* c, StreamSet& S, const std::vector<StreamRec*>& act, const StepBuild& b, OutBuild& ob, StepBuffers& B) {
    int rc;
    B.base[kRawCur] = S.barena[S.bcur].p;
    if ((rc = grow(c, S.barena[S.bcur ^ 1], B, kRawNext)) || (rc = grow(c, S.d_out, B, kOut)) || (rc = S.h_out.reserve(c, B.need[kOut])) || (rc = grow(c, S.d_outb, B, kOutb)) ||
        (rc = B.need[kOutb] ? S.h_outb.reserve(c, B.need[kOutb]) : SS_OK) || (rc = grow(c, S.d_up2, B, kUp2)) || (rc = S.h_up2.reserve(c, B.need[kUp2])))
        return rc;
    build_outputs(ob, act, b, B);
    // (regions of fixed room: the descriptors' range tables were addressed before the vectors were complete)
    const size_t n = ob.ops.size();
    UploadPacker pk(S.h_up2.p, B.need[kUp2]);
    const size_t o_sil = pk.put(ob.sil.data(), ob.sil.size() * sizeof(StreamSilence), n * sizeof(StreamSilence));
    const size_t o_cpb = pk.put(ob.cpb.data(), ob.cpb.size() * sizeof(StreamCopyBytes), 2 * n * sizeof(StreamCopyBytes));
    const size_t o_src = pk.put(ob.srcs.data(), ob.srcs.size() * sizeof(StreamSilenceSource), n * sizeof(StreamSilenceSource));
    if (pk.put(ob.rng_all) != (size_t)output_ranges_off(n)) pk.ok = false;
    if ((rc = upload(c, pk, S.d_up2.p, pk.used, "output's"))) return rc;
    {
        ScopedLaunch sl(c, c->stream, "stream_silence_kernel", 0.0, ob.in_bytes + 2.0 * (double)ob.total_out);
        HIPCHK(c, launch_stream_silence((const StreamSilence*)(S.d_up2.p + o_sil), (int)ob.sil.size(), ob.max_samples, S.d_out.p, c->stream));
    }
    if (!ob.srcs.empty()) {        // (the copy of the carried PCM below writes the other half of the byte arena: either order will do)
        ScopedLaunch sl(c, c->stream, "stream_silence_source_kernel", 0.0, 2.0 * ob.src_bytes);
        HIPCHK(c, launch_stream_silence_source((const StreamSilenceSource*)(S.d_up2.p + o_src), (int)ob.srcs.size(), ob.max_src, S.d_outb.p, c->stream));
    }
    {
        ScopedLaunch sl(c, c->stream, "stream_copy_bytes", 0.0, 2.0 * ob.carried);
        HIPCHK(c, launch_stream_copy_bytes((const StreamCopyBytes*)(S.d_up2.p + o_cpb), (int)ob.cpb.size(), ob.max_bytes, c->stream));
    }
    if (!ob.sil.empty()) HIPCHK(c, hipMemcpyAsync(S.h_out.p, S.d_out.p, (size_t)ob.total_out * 2, hipMemcpyDeviceToHost, c->stream));
    if (!ob.srcs.empty()) HIPCHK(c, hipMemcpyAsync(S.h_outb.p, S.d_outb.p, (size_t)ob.total_outb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    return SS_OK;
}

extern "C" int ss_stream_step(ss_ctx* c) {
    if (!c) return fail(nullptr, SS_ERR_ARG, "null context");
    if (!c->has_model) return fail(c, SS_ERR_STATE, "context was created without weights (audio-only)");
    if (c->run_pending) return fail(c, SS_ERR_STATE, "a run is in flight: ss_run_end first");
    hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (the pinned upload buffer is rewritten below)
    StreamSet& S = streams_of(c);
    int rc;
    std::vector<StreamRec*> act;                            // every unfinished stream
    for (auto& kv : S.s) if (!kv.second.finished) act.push_back(&kv.second);
    StepBuffers B;
    StepBuild b = plan_step(act, c->chunk, B);
    if ((rc = run_step(c, S, act, b, B))) return rc;
    commit_step(S.s, act, b, S.h_avg.data(), S.h_flags.data());
    S.cur ^= 1;                                             // (the records describe the half just built from here on)
    if (b.n_band_lanes) {
        const BandBuild bb = layout_bands(act, b, B);
        if ((rc = run_bands(c, S, bb, B))) return rc;
        commit_bands(act, (const ss_region_band*)S.h_bres.p, (const double*)(S.h_bres.p + bb.rec_bytes));
    }
    OutBuild ob = plan_outputs(act, B);
    if (ob.ops.empty()) return SS_OK;
    if ((rc = run_output(c, S, act, b, ob, B))) return rc;
    commit_outputs(act, ob);
    S.bcur ^= 1;
    return SS_OK;
}

// ------------------------------------------------------------------------------------------------------
// export / import: a stream's whole state as a byte image
// ------------------------------------------------------------------------------------------------------
namespace {
struct ImageHdr {
    char magic[8];
    int32_t format, sr, ch, closed, finished, have, run_open, pad;
    double thr, brk, cur_start, cur_end;
    int64_t frames_in, staged_frames, staged_bytes, mono_base, mono_n, sig_base, sig_n, lg_w0, lg_n, m_next, win_run, bins_done, run_first, run_last;
};
// "SSSTRM01": a stream with the default window step -- the header, then the data.  "SSSTRM02": any other step -- the header, the step
// (a double), then the data.
constexpr char kMagic[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '1'};
constexpr char kMagicStep[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '2'};
// "SSSTRM03": a stream with output -- the header, the step, ImageOut, n_er int64s (the decided ranges still ahead), the staged bytes,
// the floats, then the held raw PCM (raw_bytes: frames [frames_out, frames_in) in the stream's encoding)
constexpr char kMagicOut[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '3'};
struct ImageOut { double pad_s, min_len_s; int64_t frames_out, erased, raw_bytes, n_er; };
// "SSSTRM04": an each-channel stream of several channels -- the header, the step, ImageLanes, the peak state (3 x lanes doubles: open
// run, pending region, gap), then with_out ? the output block of "SSSTRM03" (ImageOut, the ranges) : nothing, the staged bytes, the
// floats (every lane's mono history, then every lane's signal, then every lane's logits), then the held raw PCM of a stream with output
constexpr char kMagicLanes[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '4'};
struct ImageLanes { int32_t lanes, with_out; };
// "SSSTRM05": a stream with bands (of any other kind: mix or each-channel, with or without output) -- the header, the step (the default
// one: bands know no other), ImageBands, lanes > 1 ? the peak state of "SSSTRM04" : nothing, with_out ? the output block of "SSSTRM03" :
// nothing, the staged bytes, the floats as in "SSSTRM04", the band state as doubles (every lane's accumulator vectors [kBandAcc][256],
// then every lane's map sums [256][bs_n] of the bins [bins_done, bins_done + bs_n)), then the held raw PCM of a stream with output
constexpr char kMagicBands[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '5'};
struct ImageBands { int32_t lanes, with_out, want_prof, parked, speech_channel, reserved; double q_low, q_high; int64_t bs_n; };
// "SSSTRM06": a stream with output in its own encoding (ss_stream_open_source) -- these eight bytes, then the image the stream would
// write without that property ("SSSTRM03" or "SSSTRM04"), whole
constexpr char kMagicSource[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '6'};
constexpr int64_t kMaxCarriedBins = 4096;             // (a stream carries the sums of about 300 bins)
}  // namespace

static int export_image(ss_ctx* c, StreamRec* s, void* buf, int64_t cap, int64_t* n_out);
static int import_image(ss_ctx* c, const void* buf, int64_t n, int* id);

extern "C" int ss_stream_export(ss_ctx* c, int id, void* buf, int64_t cap, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_export: bad argument");
    if (!s->src_out) return export_image(c, s, buf, cap, n_out);
    int rc = export_image(c, s, buf ? (unsigned char*)buf + 8 : nullptr, buf ? std::max<int64_t>(cap - 8, 0) : 0, n_out);
    *n_out += 8;
    if (rc == SS_OK && buf) memcpy(buf, kMagicSource, 8);
    return rc;
}

extern "C" int ss_stream_import(ss_ctx* c, const void* buf, int64_t n, int* id) {
    if (!c || !buf || !id || n < (int64_t)sizeof(ImageHdr)) return fail(c, SS_ERR_ARG, "ss_stream_import: bad argument");
    if (memcmp(buf, kMagicSource, 8) != 0) return import_image(c, buf, n, id);
    const unsigned char* inner = (const unsigned char*)buf + 8;
    if (n < 8 + (int64_t)sizeof(ImageHdr) || (memcmp(inner, kMagicOut, 8) != 0 && memcmp(inner, kMagicLanes, 8) != 0))
        return fail(c, SS_ERR_FORMAT, "ss_stream_import: not a stream image");
    int rc = import_image(c, inner, n - 8, id);
    if (rc) return rc;
    StreamRec* s = find_stream(c, *id);
    if (!s->out_on) { ss_stream_free(c, *id); return fail(c, SS_ERR_FORMAT, "ss_stream_import: a source-output image of a stream without output"); }
    s->src_out = true;
    return SS_OK;
}

static int export_image(ss_ctx* c, StreamRec* s, void* buf, int64_t cap, int64_t* n_out) {
    const bool each = s->lanes > 1, bands = s->bands_on;
    const bool with_step = bands || each || s->out_on || s->step != SS_STEP_DEFAULT;
    const int64_t band_doubles = bands ? (int64_t)s->lanes * 256 * (kBandAcc + s->bs_n) : 0;
    const int64_t raw_bytes = s->out_on ? (s->frames_in - s->frames_out) * s->frame_bytes() : 0;
    const int64_t nl = s->lanes;
    const int64_t need = (int64_t)sizeof(ImageHdr) + (with_step ? 8 : 0) + (bands ? (int64_t)sizeof(ImageBands) : each ? (int64_t)sizeof(ImageLanes) : 0) +
                         (each ? 24 * nl : 0) + (int64_t)s->staged.size() + 4 * nl * (s->mono_n + s->sig_n + s->lg_n * 256) + 8 * band_doubles +
                         (s->out_on ? (int64_t)sizeof(ImageOut) + 8 * (int64_t)s->er_rng.size() + raw_bytes : 0);
    *n_out = need;
    if (!buf) return SS_OK;
    if (cap < need) return fail(c, SS_ERR_CAPACITY, "ss_stream_export: capacity < " + std::to_string(need));
    ImageHdr h{};
    memcpy(h.magic, bands ? kMagicBands : each ? kMagicLanes : s->out_on ? kMagicOut : with_step ? kMagicStep : kMagic, 8);
    h.format = s->format; h.sr = s->sr; h.ch = s->ch; h.closed = s->closed; h.finished = s->finished; h.have = s->mg.have; h.run_open = s->run_open;
    h.thr = s->thr; h.brk = s->mg.brk; h.cur_start = s->mg.cur.start; h.cur_end = s->mg.cur.end;
    h.frames_in = s->frames_in; h.staged_frames = s->staged_frames; h.staged_bytes = (int64_t)s->staged.size();
    h.mono_base = s->mono_base; h.mono_n = s->mono_n; h.sig_base = s->sig_base; h.sig_n = s->sig_n; h.lg_w0 = s->lg_w0; h.lg_n = s->lg_n;
    h.m_next = s->m_next; h.win_run = s->win_run; h.bins_done = s->bins_done; h.run_first = s->run_first; h.run_last = s->run_last;
    unsigned char* o = (unsigned char*)buf;
    memcpy(o, &h, sizeof h); o += sizeof h;
    if (with_step) { memcpy(o, &s->step, 8); o += 8; }
    if (bands) {
        const ImageBands ib{s->lanes, s->out_on ? 1 : 0, s->want_prof ? 1 : 0, s->b_parked ? 1 : 0, s->bprm.speech_channel, 0, s->bprm.q_low, s->bprm.q_high, s->bs_n};
        memcpy(o, &ib, sizeof ib); o += sizeof ib;
    } else if (each) {
        const ImageLanes il{s->lanes, s->out_on ? 1 : 0};
        memcpy(o, &il, sizeof il); o += sizeof il;
    }
    if (each) {
        for (const std::vector<double>* v : {&s->pk_run, &s->pk_cur, &s->pk_gap}) { memcpy(o, v->data(), 8 * nl); o += 8 * nl; }
    }
    if (s->out_on) {
        const ImageOut io{s->er.pad_s, s->er.min_len_s, s->frames_out, s->erased, raw_bytes, (int64_t)s->er_rng.size()};
        memcpy(o, &io, sizeof io); o += sizeof io;
        if (!s->er_rng.empty()) memcpy(o, s->er_rng.data(), s->er_rng.size() * 8);
        o += s->er_rng.size() * 8;
    }
    if (!s->staged.empty()) memcpy(o, s->staged.data(), s->staged.size());
    o += s->staged.size();
    float* f = (float*)o;                                 // (unaligned host memory is fine for memcpy / hipMemcpy)
    unsigned char* bnd = o + 4 * nl * (s->mono_n + s->sig_n + s->lg_n * 256);        // (doubles at any alignment: written by memcpy only)
    unsigned char* raw = bnd + 8 * band_doubles;
    float* f_sig = f + nl * s->mono_n; float* f_lg = f_sig + nl * s->sig_n;       // the lanes back to back, as the host vectors hold them
    if (s->on_host) {
        memcpy(f, s->h_mono.data(), nl * s->mono_n * 4); memcpy(f_sig, s->h_sig.data(), nl * s->sig_n * 4);
        memcpy(f_lg, s->h_lg.data(), nl * s->lg_n * 1024);
        if (raw_bytes) memcpy(raw, s->h_raw.data(), (size_t)raw_bytes);
        if (band_doubles) memcpy(bnd, s->h_band.data(), (size_t)band_doubles * 8);
        return SS_OK;
    }
    hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const float* a = c->streams->arena[c->streams->cur].p;
    for (int64_t l = 0; l < nl; ++l) {
        if (s->mono_n) HIPCHK(c, hipMemcpy(f + l * s->mono_n, a + s->mono_off + l * s->mono_ls, s->mono_n * 4, hipMemcpyDeviceToHost));
        if (s->sig_n) HIPCHK(c, hipMemcpy(f_sig + l * s->sig_n, a + s->sig_off + l * s->sig_ls, s->sig_n * 4, hipMemcpyDeviceToHost));
        if (s->lg_n) HIPCHK(c, hipMemcpy(f_lg + l * s->lg_n * 256, a + s->lg_off + l * s->lg_ls, s->lg_n * 1024, hipMemcpyDeviceToHost));
    }
    if (raw_bytes) HIPCHK(c, hipMemcpy(raw, c->streams->barena[c->streams->bcur].p + s->raw_off, (size_t)raw_bytes, hipMemcpyDeviceToHost));
    if (bands && !s->bs_ls) memset(bnd, 0, (size_t)band_doubles * 8);                  // no step yet: nothing carried, the accumulators zero
    else if (bands) {
        unsigned char* sums = bnd + (size_t)nl * 256 * kBandAcc * 8;
        for (int64_t l = 0; l < nl; ++l) {
            const float* lane = a + s->bs_off + l * s->bs_ls;
            HIPCHK(c, hipMemcpy(bnd + (size_t)l * 256 * kBandAcc * 8, lane, 256 * kBandAcc * 8, hipMemcpyDeviceToHost));
            if (s->bs_n)
                HIPCHK(c, hipMemcpy2D(sums + (size_t)l * 256 * s->bs_n * 8, (size_t)s->bs_n * 8, lane + s->bs_sum_off, (size_t)s->bs_stride * 8, (size_t)s->bs_n * 8, 256,
                                      hipMemcpyDeviceToHost));
        }
    }
    return SS_OK;
}

static int import_image(ss_ctx* c, const void* buf, int64_t n, int* id) {
    if (!c || !buf || !id || n < (int64_t)sizeof(ImageHdr)) return fail(c, SS_ERR_ARG, "ss_stream_import: bad argument");
    if (!c->has_model) return fail(c, SS_ERR_STATE, "context was created without weights (audio-only)");
    ImageHdr h;
    memcpy(&h, buf, sizeof h);
    static const unsigned char one[8] = {0};
    // an "SSSTRM04" image that does not hold together is an argument error (SS_ERR_ARG); the older images keep SS_ERR_FORMAT
    const bool bands = memcmp(h.magic, kMagicBands, 8) == 0;
    const bool each = bands || memcmp(h.magic, kMagicLanes, 8) == 0;    // (the lanes' block: ImageLanes, or ImageBands which begins like it)
    const int bad = each ? SS_ERR_ARG : SS_ERR_FORMAT;
    bool with_out = memcmp(h.magic, kMagicOut, 8) == 0;
    const bool with_step = each || with_out || memcmp(h.magic, kMagicStep, 8) == 0;
    int64_t hdr_bytes = (int64_t)sizeof h;
    double step = SS_STEP_DEFAULT;
    if (with_step && n >= hdr_bytes + 8) { memcpy(&step, (const unsigned char*)buf + hdr_bytes, 8); hdr_bytes += 8; }
    ImageLanes il{1, 0};
    ImageBands ib{1, 0, 0, 0, 1, 0, 0.05, 0.95, 0};
    int64_t pk_at = 0;                                    // the peak state's place in the image
    if (each) {
        const int64_t blk = bands ? (int64_t)sizeof ib : (int64_t)sizeof il;
        bool ok = hdr_bytes == (int64_t)sizeof h + 8 && n >= hdr_bytes + blk;
        if (ok) {
            memcpy(&il, (const unsigned char*)buf + hdr_bytes, sizeof il);
            const int64_t pk = !bands || il.lanes > 1 ? 24 * (int64_t)il.lanes : 0;       // (an "SSSTRM04" image always holds the peak block)
            ok = il.lanes >= 1 && (il.lanes == 1 || il.lanes == h.ch) && il.lanes <= 64 && (il.with_out == 0 || il.with_out == 1) && n >= hdr_bytes + blk + pk;
            if (ok && bands) {
                memcpy(&ib, (const unsigned char*)buf + hdr_bytes, sizeof ib);
                const ss_band_params bp{ib.q_low, ib.q_high, ib.speech_channel, 0};
                std::string err;
                ok = (ib.want_prof == 0 || ib.want_prof == 1) && (ib.parked == 0 || ib.parked == 1) && ib.reserved == 0 && ib.bs_n >= 0 && ib.bs_n <= kMaxCarriedBins &&
                     check_band_args(nullptr, 0, &bp, err) == SS_OK && step == SS_STEP_DEFAULT;
            }
            pk_at = hdr_bytes + blk;
            hdr_bytes = pk_at + pk;
        }
        if (!ok)
            return fail(c, SS_ERR_ARG, bands ? "ss_stream_import: a band image that does not hold together (lane count, parameters, a step other than the default, or cut short)"
                                             : "ss_stream_import: an each-channel image whose lane count is neither 1 nor its channel count, or cut short");
        with_out = il.with_out != 0;
    }
    const int64_t nl = il.lanes;
    const int64_t band_bytes = bands ? 8 * nl * 256 * (kBandAcc + ib.bs_n) : 0;
    ImageOut io{0, 0, 0, 0, 0, 0};
    int64_t out_bytes = 0;                                // what an image with output holds beyond the others: ImageOut, the ranges, the raw PCM
    if (with_out) {
        bool ok = n >= hdr_bytes + (int64_t)sizeof io;
        if (ok) {
            memcpy(&io, (const unsigned char*)buf + hdr_bytes, sizeof io);
            const ss_stream_erase e{io.pad_s, io.min_len_s};
            ok = erase_ok(&e) && io.n_er >= 0 && io.n_er <= ((int64_t)1 << 24) && io.n_er % 2 == 0 && io.frames_out >= 0 && io.frames_out <= h.frames_in &&
                 io.erased >= 0 && io.erased <= io.frames_out && h.ch > 0 && h.ch <= 64 && io.raw_bytes >= 0 && io.raw_bytes <= n;
        }
        if (!ok) return fail(c, bad, "ss_stream_import: not a stream image");
        hdr_bytes += (int64_t)sizeof io + 8 * io.n_er;
        out_bytes = io.raw_bytes;
    }
    if ((memcmp(h.magic, kMagic, 8) != 0 && !(with_step && hdr_bytes > (int64_t)sizeof h && step_ok(step))) || check_pcm_args(c, one, h.format, h.sr, h.ch, 0) != SS_OK || h.staged_bytes < 0 || h.mono_n < 0 ||
        h.sig_n < 0 || h.lg_n < 0 || h.lg_n > 64 || h.mono_n > ((int64_t)1 << 32) || h.sig_n > ((int64_t)1 << 32) ||
        n != hdr_bytes + h.staged_bytes + 4 * nl * (h.mono_n + h.sig_n + h.lg_n * 256) + band_bytes + out_bytes ||
        (with_out && io.raw_bytes != (h.frames_in - io.frames_out) * h.ch * (int64_t)pcm_bytes_per_sample(h.format)) ||
        h.staged_bytes != h.staged_frames * h.ch * (int64_t)pcm_bytes_per_sample(h.format))
        return fail(c, bad, "ss_stream_import: not a stream image");
    hipSetDevice(c->device);
    StreamRec s;
    s.format = h.format; s.sr = h.sr; s.ch = h.ch; s.closed = h.closed; s.finished = h.finished; s.mg.have = h.have; s.run_open = h.run_open;
    s.thr = h.thr; s.mg.brk = h.brk; s.mg.cur = ss_region{h.cur_start, h.cur_end};
    s.step = step; s.per_step = step_samples(step);
    s.frames_in = h.frames_in; s.staged_frames = h.staged_frames;
    s.mono_base = h.mono_base; s.mono_n = h.mono_n; s.sig_base = h.sig_base; s.sig_n = h.sig_n; s.lg_w0 = h.lg_w0; s.lg_n = h.lg_n;
    s.m_next = h.m_next; s.win_run = h.win_run; s.bins_done = h.bins_done; s.run_first = h.run_first; s.run_last = h.run_last;
    int rc = init_rates(c, s);
    if (rc) return rc;
    const unsigned char* p = (const unsigned char*)buf + hdr_bytes;
    s.staged.assign(p, p + h.staged_bytes); p += h.staged_bytes;
    s.set_lanes((int)nl);
    if (nl > 1)
        for (std::vector<double>* v : {&s.pk_run, &s.pk_cur, &s.pk_gap}) { memcpy(v->data(), (const unsigned char*)buf + pk_at, 8 * nl); pk_at += 8 * nl; }
    s.h_mono.resize(nl * h.mono_n); s.h_sig.resize(nl * h.sig_n); s.h_lg.resize(nl * h.lg_n * 256);
    memcpy(s.h_mono.data(), p, nl * h.mono_n * 4); p += nl * h.mono_n * 4;
    memcpy(s.h_sig.data(), p, nl * h.sig_n * 4); p += nl * h.sig_n * 4;
    memcpy(s.h_lg.data(), p, nl * h.lg_n * 1024); p += nl * h.lg_n * 1024;
    if (bands) {
        s.bands_on = true; s.want_prof = ib.want_prof != 0; s.b_parked = ib.parked != 0; s.bprm = ss_band_params{ib.q_low, ib.q_high, ib.speech_channel, 0};
        s.bs_n = ib.bs_n;
        s.h_band.resize((size_t)(band_bytes / 8));
        memcpy(s.h_band.data(), p, (size_t)band_bytes); p += band_bytes;
    }
    if (with_out) {
        s.out_on = true; s.er = ss_stream_erase{io.pad_s, io.min_len_s}; s.frames_out = io.frames_out; s.erased = io.erased;
        const unsigned char* q = (const unsigned char*)buf + hdr_bytes - 8 * io.n_er;
        s.er_rng.resize((size_t)io.n_er);
        if (io.n_er) memcpy(s.er_rng.data(), q, (size_t)io.n_er * 8);
        s.h_raw.assign(p, p + io.raw_bytes);
        s.o_first = s.frames_out;
    }
    s.on_host = true;
    StreamSet& S = streams_of(c);
    *id = S.next_id++;
    S.s.emplace(*id, std::move(s));
    return SS_OK;
}
