// The descriptors of the stream kernels (frontend.hip's stream_* kernels, stream.hip's stream_map_kernel and stream_band_kernel): one
// launch per step for all streams, a descriptor per stream or lane; and those of the ingest kernels (ingest.hip), one per file or
// recording of a batch.  Plain data, no HIP header: the host-only plans (stream_plan.h, ingest_plan.h) build them, and
// tests/stream_extents.cpp and tests/ingest_plan_check.cpp check what they address without a device.
#pragma once
#include <cstdint>

namespace ss {

// ---- ingest ----
// a file of a batch: its bytes at pcm + pcm_off; decoded (and mixed down) to mono[mono_off ..), resampled to arena[out_off .. + n_out)
struct BatchFile { int64_t pcm_off; int64_t frames; int64_t mono_off; int64_t out_off; int64_t n_out; };
// per-channel ingest (no mixdown): channel c of a recording is decoded to dst[mono_off + c mono_stride ..) / resampled to
// arena[out_off + c out_stride ..); one descriptor per recording, the channels' planes a constant stride apart
struct ChanFile { int64_t pcm_off; int64_t frames; int64_t mono_off; int64_t out_off; int64_t n_out; int64_t mono_stride; int64_t out_stride; };

// ---- streams ----
struct StreamCopy { const float* src; float* dst; int64_t n; };                       // src == nullptr: n zeros
struct StreamDecode { int64_t pcm_off; int64_t frames; float* dst; int32_t format, channels; };
// outputs [m0, m0 + n) -> out[0 .. n); input sample idx is mono[idx - mono_base] for mono_base <= idx < frames, zero past `frames`
struct StreamResample { const float* mono; int64_t mono_base, frames; const float* taps; float* out; int64_t m0, n; int32_t L, M, half, pad; };
// bins [b0, b0 + nb) from the windows [w0, W) whose logits lie back to back at `logits`; results at avg / flags [out_off ..); step: the
// stream's window step in seconds (window i starts at bin rint(i step / (3 / 256)), as ss_window_start_bin), s_b = step x 256 / 3
struct StreamAvg { const float* logits; int64_t w0; int32_t W, pad; int64_t b0, nb, out_off; double threshold, step, s_b; };
// streaming silencer: frames [frame0, frame0 + n) of a stream -> out[out_off ..) as interleaved int16; the first n0 frames are read from
// seg0, the others from seg1 (native encoding, each aligned to a sample); frames inside ranges (n_ranges disjoint ascending [begin, end)
// pairs of recording frame numbers) are zero
struct StreamSilence { const unsigned char* seg0; const unsigned char* seg1; const int64_t* ranges; int64_t n0, frame0, n, out_off;
                       int32_t n_ranges, format, channels, pad; };
struct StreamCopyBytes { const unsigned char* src; unsigned char* dst; int64_t n; };   // n bytes, any alignment
// streaming silencer in the stream's own encoding: bytes [byte0, byte0 + n) of the recording -> out[out_off ..) (out_off a multiple of 16);
// the first n0 bytes are read from seg0, the others from seg1, at any alignment; bytes inside ranges (n_ranges disjoint ascending
// [begin, end) pairs of recording BYTE numbers) become the zero byte (zero4: it, four times)
struct StreamSilenceSource { const unsigned char* seg0; const unsigned char* seg1; const int64_t* ranges; int64_t n0, byte0, n, out_off;
                             int32_t n_ranges; uint32_t zero4; };
// each-channel streams (ss_stream_open_channels): the pushed frames of a stream of `channels` lanes -> channel c's samples at
// dst[c stride ..), no mean; pcm_off is a multiple of 16 (the fast form reads a 16-bit stereo frame as one 32-bit word)
struct StreamDecodeChannels { int64_t pcm_off; int64_t frames; float* dst; int64_t stride; int32_t format, channels; };
// the merged series of such a stream: its `lanes` lanes' nb new bins lie at avg / flags [in_off + l nb ..); the OR of the flag bits and
// the fmax of the averages (a NaN passed over) go to avg / flags [out_off ..)
struct StreamUnion { int64_t in_off, nb, out_off; int32_t lanes, pad; };

// ---- bands ----
constexpr int kBandAcc = 5;                           // 256-double vectors per lane: done, cur, snap_done, snap_cur, parked
enum { kEvReset = 0, kEvSnap = 1, kEvPark = 2, kEvEmitSnap = 3, kEvEmitPark = 4 };
// one decision of the host's region walk.  Reset / snap act before bin `pos` is added: reset clears both accumulators (a candidate region
// starts at pos), snap copies them (the candidate's bins end before pos).  Park forms the snapshot's profile and sets it aside (the region
// is final, the walk returns it later); emit evaluates record `rec` of the step (n_bins bins) from the snapshot or from the parked vector.
struct StreamBandEv { int64_t pos; int32_t type, n_bins; int64_t rec; };
// one launch's work on one band lane's map sums [256][stride] over the bins [b0, b0 + n) of the step.  Flags: kMapInit -- the sums start
// from the carried ones and zeros (the lane's first entry of the step); the windows [i0, i1) of this pass, the first at spec slot slot0,
// are added (none when i0 == i1); kMapFin -- the first fin_n bins become float32 maps fmap [256][fin_n] (the lane's last entry)
enum { kMapInit = 1, kMapFin = 2 };
struct StreamMap {
    const double* old_sum; int64_t old_stride, old_b0, old_n;
    double* sum; int64_t stride, b0, n;
    int64_t i0, i1, slot0;
    float* fmap; int64_t fin_n, i_end;
    int32_t flags, pad;
};
// one band lane's walk over the step's final bins [b0, b0 + nb) (fmap [256][nb]) under the stream's events ev0 .. ev0 + nev - 1
struct StreamBand {
    const double* acc_old; double* acc;
    const float* fmap; int64_t b0, nb;
    int64_t out0;                                     // record (rec, lane) of the stream: out0 + rec lanes + lane
    int32_t ev0, nev, lanes, lane, speech_ch, want_prof;
    double q_low, q_high;
};

}  // namespace ss
