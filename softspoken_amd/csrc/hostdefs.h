// Host-only rules and types the units of the library share: sample sizes, the run merger, bin times and window steps, rule 1 of the
// region bands, the silencer's frame ranges, the erase table's filter.  No HIP header: engine.h includes this, and so do stream_plan.h
// and sep_plan.h, which have to compile without a device toolchain.  Defined in host.hip.
#pragma once
#include "../../include/softspoken.h"

#include <cstdint>
#include <vector>

namespace ss {

// bytes of one sample of enum ss_pcm_format (WAV: little endian; AIFF: big endian, 7..12)
inline size_t pcm_bytes_per_sample(int format) {
    switch (format) {
        case SS_PCM_U8: case SS_PCM_S8: return 1;
        case SS_PCM_S16: case SS_PCM_S16BE: return 2;
        case SS_PCM_S24: case SS_PCM_S24BE: return 3;
        case SS_PCM_F64: case SS_PCM_F64BE: return 8;
        default: return 4;
    }
}

// Gap merge of runs of bins above the threshold, in bin order (NNDetector.py:131-141, then worker.py:100's shift by the 3 s of padding):
// a run whose start lies at most brk seconds behind the current region's end extends it, any other run emits the region and opens the
// next.  bins (optional): first and last bin of every emitted region.  The callers keep their own scans for the runs.
struct RunMerger {
    double brk = 0; bool have = false; ss_region cur{0, 0}; int64_t reg0 = 0, reg1 = 0;
    void add(int64_t first_bin, int64_t last_bin, std::vector<ss_region>& out, std::vector<int64_t>* bins = nullptr);
    void flush(std::vector<ss_region>& out, std::vector<int64_t>* bins = nullptr);      // emits the current region, if any
};

void region_bins(double start, double end, int64_t lo, int64_t hi, int64_t& first, int64_t& count);   // rule 1, clamped to [lo, hi)
std::vector<int64_t> silence_ranges(const ss_region* regions, int64_t n, int sr, int64_t frames);   // merged frame ranges [begin, end) of a region table
double bin_time(int64_t idx);                             // float(f"{idx / (256 / 3):.4f}")
bool step_ok(double step_s);                              // a window step ss_set_window_step accepts
int64_t step_samples(double step_s);                      // floor(22050 step): samples between window starts
inline double step_bins(double step_s) { return step_s * 256.0 / 3.0; }   // s_b: bins between window starts, before the rounding of a start
// the streaming silencer's erase table (ss_erase_table): the length filter and the padding of one region of the table
bool erase_ok(const ss_stream_erase* e);                  // NULL, or both parameters finite and >= 0
inline bool erase_keeps(const ss_region& r, double min_len_s) { return !(r.end - r.start <= min_len_s); }
inline ss_region erase_padded(const ss_region& r, double pad_s) { return ss_region{r.start - pad_s, r.end + pad_s}; }

}  // namespace ss
