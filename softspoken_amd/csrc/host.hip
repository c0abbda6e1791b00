// Host-only pieces of the path (no device work): RIFF/WAVE header walk, window plan, threshold / run-length / gap-merge, the
// reference's time strings and CSV text, rule 1 of the region bands, silencer frame ranges, WAV header writer.  Reference lines are cited per function.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace ss;

// voice_activity.py:23-30 (get_audio_data) needs duration + native rate; load_audio needs the samples.
// AIFF / AIFF-C ("FORM" size "AIFF" | "AIFC"; big-endian chunk sizes): COMM = channels u16, frames u32, bits u16, sample rate as an 80-bit
// extended float [, compression type, name]; SSND = offset u32, block size u32, samples.  8-bit samples are signed.
static int aiff_parse(const unsigned char* b, size_t nbytes, ss_wav_info* out) {
    auto be16 = [&](size_t p) { return (uint32_t)b[p] << 8 | b[p + 1]; };
    auto be32 = [&](size_t p) { return (uint32_t)b[p] << 24 | (uint32_t)b[p + 1] << 16 | (uint32_t)b[p + 2] << 8 | b[p + 3]; };
    const bool aifc = memcmp(b + 8, "AIFC", 4) == 0;
    size_t pos = 12;
    bool have_comm = false;
    uint32_t ch = 0, bits = 0, n_frames = 0; double sr = 0; char comp[5] = "NONE";
    while (pos + 8 <= nbytes) {
        const uint32_t sz = be32(pos + 4);
        const size_t body = pos + 8;
        if (memcmp(b + pos, "COMM", 4) == 0) {
            if (sz < 18 || body + 18 > nbytes) return fail(nullptr, SS_ERR_FORMAT, "AIFF: short COMM chunk");
            ch = be16(body); n_frames = be32(body + 2); bits = be16(body + 6);
            const int e = (int)(be16(body + 8) & 0x7fff) - 16383;                  // 80-bit extended: sign + 15-bit exponent, 64-bit mantissa with its leading 1
            const uint64_t mant = (uint64_t)be32(body + 10) << 32 | be32(body + 14);
            sr = (be16(body + 8) & 0x7fff) == 0x7fff ? 0.0 : std::ldexp((double)mant, e - 63);
            if (aifc) {
                if (sz < 22 || body + 22 > nbytes) return fail(nullptr, SS_ERR_FORMAT, "AIFF-C: COMM chunk without a compression type");
                memcpy(comp, b + body + 18, 4);
            }
            have_comm = true;
        } else if (memcmp(b + pos, "SSND", 4) == 0) {
            if (!have_comm) return fail(nullptr, SS_ERR_FORMAT, "AIFF: SSND chunk before COMM chunk");
            if (sz < 8 || body + 8 > nbytes) return fail(nullptr, SS_ERR_FORMAT, "AIFF: short SSND chunk");
            const uint32_t off = be32(body);
            int fmt = 0;
            const bool le = memcmp(comp, "sowt", 4) == 0;
            if (memcmp(comp, "NONE", 4) == 0 || le) {
                if (bits == 8) fmt = SS_PCM_S8;
                else if (bits == 16) fmt = le ? SS_PCM_S16 : SS_PCM_S16BE;
                else if (bits == 24) fmt = le ? SS_PCM_S24 : SS_PCM_S24BE;
                else if (bits == 32) fmt = le ? SS_PCM_S32 : SS_PCM_S32BE;
            } else if (memcmp(comp, "fl32", 4) == 0 || memcmp(comp, "FL32", 4) == 0) { fmt = SS_PCM_F32BE; bits = 32; }
            else if (memcmp(comp, "fl64", 4) == 0 || memcmp(comp, "FL64", 4) == 0) { fmt = SS_PCM_F64BE; bits = 64; }
            if (!fmt) return fail(nullptr, SS_ERR_FORMAT, std::string("AIFF: unsupported encoding (") + comp + ", " + std::to_string(bits) + " bits)");
            if (ch == 0 || !(sr >= 1.0) || sr > 2147483647.0) return fail(nullptr, SS_ERR_FORMAT, "AIFF: zero channels or sample rate out of range");
            if ((uint64_t)body + 8 + off > nbytes) return fail(nullptr, SS_ERR_FORMAT, "AIFF: SSND offset beyond the file");
            const size_t start = body + 8 + off;
            const size_t avail = std::min<size_t>(sz - 8 > off ? sz - 8 - off : 0, nbytes - start);
            const size_t fb = (size_t)ch * bits / 8;
            out->format = fmt; out->channels = (int32_t)ch; out->sample_rate = (int32_t)std::nearbyint(sr); out->bits = (int32_t)bits;
            out->data_offset = (int64_t)start; out->data_bytes = (int64_t)avail;
            out->frames = (int64_t)std::min<size_t>(avail / fb, n_frames);           // (COMM's count is the truth; a truncated file has fewer)
            return SS_OK;
        }
        pos = body + sz + (sz & 1);
    }
    return fail(nullptr, SS_ERR_FORMAT, "AIFF: missing COMM or SSND chunk");
}

extern "C" int ss_wav_parse(const void* file_bytes, size_t nbytes, ss_wav_info* out) {
    if (!file_bytes || !out) return fail(nullptr, SS_ERR_ARG, "ss_wav_parse: null argument");
    const unsigned char* b = (const unsigned char*)file_bytes;
    if (nbytes >= 12 && memcmp(b, "FORM", 4) == 0 && (memcmp(b + 8, "AIFF", 4) == 0 || memcmp(b + 8, "AIFC", 4) == 0)) return aiff_parse(b, nbytes, out);
    if (nbytes < 12 || memcmp(b, "RIFF", 4) != 0 || memcmp(b + 8, "WAVE", 4) != 0) return fail(nullptr, SS_ERR_FORMAT, "not a RIFF/WAVE (or AIFF) file");
    size_t pos = 12;
    bool have_fmt = false;
    uint16_t tag = 0, ch = 0, bits = 0; uint32_t sr = 0;
    while (pos + 8 <= nbytes) {
        uint32_t sz; memcpy(&sz, b + pos + 4, 4);
        const size_t body = pos + 8;
        if (memcmp(b + pos, "fmt ", 4) == 0) {
            if (sz < 16 || body + 16 > nbytes) return fail(nullptr, SS_ERR_FORMAT, "WAV: short fmt chunk");
            memcpy(&tag, b + body, 2); memcpy(&ch, b + body + 2, 2); memcpy(&sr, b + body + 4, 4); memcpy(&bits, b + body + 14, 2);
            if (tag == 0xFFFE && sz >= 26 && body + 26 <= nbytes) memcpy(&tag, b + body + 24, 2);   // WAVE_FORMAT_EXTENSIBLE sub-format
            have_fmt = true;
        } else if (memcmp(b + pos, "data", 4) == 0) {
            if (!have_fmt) return fail(nullptr, SS_ERR_FORMAT, "WAV: data chunk before fmt chunk");
            int fmt = 0;
            if (tag == 1 && bits == 8) fmt = SS_PCM_U8;
            else if (tag == 1 && bits == 16) fmt = SS_PCM_S16;
            else if (tag == 1 && bits == 24) fmt = SS_PCM_S24;
            else if (tag == 1 && bits == 32) fmt = SS_PCM_S32;
            else if (tag == 3 && bits == 32) fmt = SS_PCM_F32;
            else if (tag == 3 && bits == 64) fmt = SS_PCM_F64;
            else return fail(nullptr, SS_ERR_FORMAT, "WAV: unsupported encoding (tag " + std::to_string(tag) + ", " + std::to_string(bits) + " bits)");
            if (ch == 0 || sr == 0) return fail(nullptr, SS_ERR_FORMAT, "WAV: zero channels or sample rate");
            if (sr > 0x7fffffffu) return fail(nullptr, SS_ERR_FORMAT, "WAV: sample rate out of range");     // (found by the header fuzz test)
            const size_t avail = std::min<size_t>(sz, nbytes - body);
            out->format = fmt; out->channels = ch; out->sample_rate = (int32_t)sr; out->bits = bits;
            out->data_offset = (int64_t)body; out->data_bytes = (int64_t)avail;
            out->frames = (int64_t)(avail / ((size_t)ch * bits / 8));
            return SS_OK;
        }
        pos = body + sz + (sz & 1);
    }
    return fail(nullptr, SS_ERR_FORMAT, "WAV: missing fmt or data chunk");
}

extern "C" int64_t ss_resampled_length(int64_t frames, int sample_rate) {
    if (sample_rate <= 0 || frames < 0) return -1;
    if (sample_rate == SS_SAMPLE_RATE) return frames;
    return (frames * SS_SAMPLE_RATE + sample_rate - 1) / sample_rate;
}

// settings.step_size (settings.py:16) as the library takes it: SS_STEP_MIN <= step <= SS_STEP_MAX, finite
bool ss::step_ok(double step_s) { return std::isfinite(step_s) && step_s >= SS_STEP_MIN && step_s <= SS_STEP_MAX; }
int64_t ss::step_samples(double step_s) { return (int64_t)std::floor(22050.0 * step_s); }   // NNDetector.py:75

// NNDetector.py:66-80
extern "C" int64_t ss_plan_windows_step(double duration_s, double step_s, int64_t* starts, int64_t cap) {
    if (!step_ok(step_s)) return -1;
    const int64_t per_step = step_samples(step_s);
    const double L = std::nearbyint(duration_s * 22050.0) + 6.0 * 22050.0;
    int64_t W = (int64_t)std::ceil((L - 66150.0) / (double)per_step);
    if (W < 0) W = 0;
    if (starts) for (int64_t i = 0; i < W && i < cap; ++i) starts[i] = i * per_step;
    return W;
}

extern "C" int64_t ss_plan_windows(double duration_s, int64_t* starts, int64_t cap) {
    return ss_plan_windows_step(duration_s, SS_STEP_DEFAULT, starts, cap);
}

// NNDetector.py:175: int(round(i * step_size / time_resolution)), Python's round (ties to even), the reference's operation order
extern "C" int64_t ss_window_start_bin(int64_t i, double step_s) {
    if (!step_ok(step_s) || i < 0) return -1;
    return (int64_t)std::nearbyint(((double)i * step_s) / (3.0 / 256.0));
}

double ss::bin_time(int64_t idx) {    // float(f"{idx / (256 / 3):.4f}")  (NNDetector.py:185, worker.py:100)
    // idx * 3 / 256 = idx * 1171875 / 1e8 exactly; the double the reference formats is within 1e-12 of it, so unless the
    // exact value is a tie at the 4th decimal the rounding is decided by integers, and q / 1e4 in double is what strtod of
    // "q.dddd" returns (both correctly rounded).  A run boundary cost two printf + strtod pairs: 1.2 ms per 256-file job.
    if (idx >= 0 && idx < ((int64_t)1 << 40)) {
        const int64_t N = idx * 1171875;
        int64_t q = N / 10000;
        const int64_t rem = N % 10000;
        if (rem != 5000) return (double)(q + (rem > 5000 ? 1 : 0)) / 10000.0;
        // a tie in exact arithmetic (every 16th index): what is formatted is the DOUBLE d = idx / (256 / 3), which lies a hair to one
        // side of the tie (q + 1/2) / 1e4 -- decide the side exactly: d = m 2^e, compare m * 20000 * 2^e with 2 q + 1 in 128-bit integers
        const double d = (double)idx / (256.0 / 3.0);
        int e; const double fr = std::frexp(d, &e);                  // d = fr * 2^e, 0.5 <= fr < 1
        const __int128 m = (__int128)std::ldexp(fr, 53); e -= 53;    // d = m * 2^e, m < 2^53 (exact)
        if (e <= 0 && e > -100) {
            const __int128 lhs = m * 20000, rhs = (__int128)(2 * q + 1) << (-e);
            if (lhs != rhs) return (double)(q + (lhs > rhs ? 1 : 0)) / 10000.0;
            return (double)(q + (q & 1)) / 10000.0;                  // the double IS the tie: round half to even, as the formatter does
        }
    }
    char buf[64];
    snprintf(buf, sizeof buf, "%.4f", (double)idx / (256.0 / 3.0));
    return strtod(buf, nullptr);
}

// rule 1 of the region bands (include/softspoken.h "region bands"): the bins whose centres lie in [start, end), clamped to the bins [lo, hi)
static int64_t band_edge_bin(double x, int64_t lo, int64_t hi) {
#pragma clang fp contract(off)
    const double s = (x + 3.0) * 256.0;
    const double q = s / 3.0;
    const double v = std::ceil(q - 0.5);
    if (!(v > (double)lo)) return lo;
    if (v >= (double)hi) return hi;
    return (int64_t)v;
}

void ss::region_bins(double start, double end, int64_t lo, int64_t hi, int64_t& first, int64_t& count) {
    first = band_edge_bin(start, lo, hi);
    count = std::max<int64_t>(0, band_edge_bin(end, lo, hi) - first);
}

// NNDetector.py:131-141 (gap merge), then worker.py:100 (the 3 s of padding in front leave the times)
void ss::RunMerger::add(int64_t first_bin, int64_t last_bin, std::vector<ss_region>& out, std::vector<int64_t>* bins) {
    const double s0 = bin_time(first_bin), e0 = bin_time(last_bin);
    if (have && s0 - cur.end <= brk) { cur.end = e0; reg1 = last_bin; return; }
    flush(out, bins);
    cur = ss_region{s0, e0}; reg0 = first_bin; reg1 = last_bin; have = true;
}
void ss::RunMerger::flush(std::vector<ss_region>& out, std::vector<int64_t>* bins) {
    if (!have) return;
    out.push_back(ss_region{cur.start - 3.0, cur.end - 3.0});
    if (bins) { bins->push_back(reg0); bins->push_back(reg1); }
    have = false;
}

// NNDetector.py:112-141 then worker.py:100
extern "C" int ss_find_regions(const double* avg, const int64_t* bin_idx, int64_t n, double threshold, double break_s,
                               ss_region* out, int64_t cap, int64_t* n_out) {
    if ((n > 0 && (!avg || !bin_idx)) || !n_out) return fail(nullptr, SS_ERR_ARG, "ss_find_regions: null argument");
    // a run's start/end are the time strings of its first/last bin: format only at run boundaries
    std::vector<ss_region> merged;
    RunMerger mg; mg.brk = break_s;
    bool open = false; int64_t first = 0, last = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (avg[i] > threshold) {
            if (!open) { first = bin_idx[i]; open = true; }
            last = bin_idx[i];
        } else if (open) { mg.add(first, last, merged); open = false; }
    }
    if (open) mg.add(first, last, merged);
    mg.flush(merged);
    *n_out = (int64_t)merged.size();
    if ((int64_t)merged.size() > cap) return fail(nullptr, SS_ERR_CAPACITY, "ss_find_regions: output capacity too small");
    if (!merged.empty()) memcpy(out, merged.data(), merged.size() * sizeof(ss_region));
    return SS_OK;
}

// "speech on any channel": the same on the element-wise fmax of the channels' series (a NaN on one channel does not hide the other; a
// bin that is NaN on all of them stays in the series, is not above and closes a run)
extern "C" int ss_find_regions_union(const double* avg, const int64_t* bin_idx, int64_t n, int n_channels, double threshold, double break_s,
                                     ss_region* out, int64_t cap, int64_t* n_out) {
    if (n_channels < 1 || n < 0 || (n > 0 && (!avg || !bin_idx)) || !n_out) return fail(nullptr, SS_ERR_ARG, "ss_find_regions_union: bad argument");
    if (n_channels == 1) return ss_find_regions(avg, bin_idx, n, threshold, break_s, out, cap, n_out);
    std::vector<double> m(avg, avg + n);
    for (int c = 1; c < n_channels; ++c)
        for (int64_t i = 0; i < n; ++i) m[i] = std::fmax(m[i], avg[(size_t)c * n + i]);
    return ss_find_regions(m.data(), bin_idx, n, threshold, break_s, out, cap, n_out);
}

// Python repr(float): shortest digits that round-trip, positional for 1e-4 <= |x| < 1e16.
static std::string py_repr(double v) {
    if (v == 0.0) return std::signbit(v) ? "-0.0" : "0.0";
    if (std::isnan(v)) return "nan";
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    char buf[64];
    int prec = 1;
    for (; prec <= 17; ++prec) { snprintf(buf, sizeof buf, "%.*e", prec - 1, v); if (strtod(buf, nullptr) == v) break; }
    std::string s(buf);
    const size_t epos = s.find('e');
    std::string mant = s.substr(0, epos);
    const int ex = atoi(s.c_str() + epos + 1);
    bool neg = false;
    if (mant[0] == '-') { neg = true; mant = mant.substr(1); }
    std::string digits;
    for (char ch : mant) if (ch != '.') digits.push_back(ch);
    std::string r;
    if (ex >= -4 && ex < 16) {
        if (ex >= 0) {
            if ((int)digits.size() <= ex + 1) r = digits + std::string(ex + 1 - digits.size(), '0') + ".0";
            else r = digits.substr(0, ex + 1) + "." + digits.substr(ex + 1);
        } else r = "0." + std::string(-ex - 1, '0') + digits;
    } else {
        r = digits.substr(0, 1);
        if (digits.size() > 1) r += "." + digits.substr(1);
        char eb[16]; snprintf(eb, sizeof eb, "e%c%02d", ex < 0 ? '-' : '+', std::abs(ex));
        r += eb;
    }
    return neg ? "-" + r : r;
}

static std::string csv_quote(const char* s) {   // csv.QUOTE_MINIMAL, as DataFrame.to_csv
    std::string v(s ? s : "");
    if (v.find_first_of(",\"\r\n") == std::string::npos) return v;
    std::string q = "\"";
    for (char ch : v) { if (ch == '"') q += "\"\""; else q.push_back(ch); }
    return q + "\"";
}

// worker.py:113-123 row dict + silencer_ui.py:816-817 to_csv(index=False)
extern "C" int64_t ss_format_csv_rows(const char* file_path, const char* file_name, const ss_region* regions, int64_t n,
                                      int64_t first_id, char* out, int64_t cap) {
    std::string s;
    const std::string fp = csv_quote(file_path), fn = csv_quote(file_name);
    for (int64_t i = 0; i < n; ++i)
        s += std::to_string(first_id + i) + "," + fp + "," + fn + "," + py_repr(regions[i].start) + "," + py_repr(regions[i].end) + ",0,,\n";
    if (out && cap > 0) {
        const size_t m = std::min<size_t>(s.size(), (size_t)cap - 1);
        memcpy(out, s.data(), m); out[m] = 0;
    }
    return (int64_t)s.size();
}
// ------------------------------------------------------------------------------------------------------
// silencer: silencer_ui.py:974-998
// ------------------------------------------------------------------------------------------------------
// Frame ranges the reference's slice assignment touches: int(round(t * sr)) with Python's round (half to
// even), clamped to [0, frames]; sorted and merged so the kernel can binary-search them.
std::vector<int64_t> ss::silence_ranges(const ss_region* regions, int64_t n, int sr, int64_t frames) {
    std::vector<std::pair<int64_t, int64_t>> r;
    for (int64_t i = 0; i < n; ++i) {
        const double a = std::nearbyint(regions[i].start * (double)sr), b = std::nearbyint(regions[i].end * (double)sr);
        if (std::isnan(a) || std::isnan(b)) continue;
        const int64_t lo = (int64_t)std::min<double>(std::max<double>(a, 0.0), (double)frames);
        const int64_t hi = (int64_t)std::min<double>(std::max<double>(b, 0.0), (double)frames);
        if (hi > lo) r.emplace_back(lo, hi);
    }
    std::sort(r.begin(), r.end());
    std::vector<int64_t> out;
    for (const auto& p : r) {
        if (!out.empty() && p.first <= out.back()) out.back() = std::max(out.back(), p.second);
        else { out.push_back(p.first); out.push_back(p.second); }
    }
    return out;
}
// ------------------------------------------------------------------------------------------------------
// streaming silencer (stream.hip): the erase table of a region table, and the frame up to which a stream's output is decided
// ------------------------------------------------------------------------------------------------------
bool ss::erase_ok(const ss_stream_erase* e) {
    return !e || (std::isfinite(e->pad_s) && std::isfinite(e->min_len_s) && e->pad_s >= 0 && e->min_len_s >= 0);
}

// E(R): the review screen's length filter on the table's own doubles (review.py:31 drops end - start <= min length; a NaN row compares
// false and stays, for silence_ranges to pass over), then pad_s on either side.  silence_ranges does the rest.
extern "C" int ss_erase_table(const ss_region* regions, int64_t n, const ss_stream_erase* erase, ss_region* out, int64_t cap, int64_t* n_out) {
    if (n < 0 || (n > 0 && !regions) || !n_out || !erase_ok(erase)) return fail(nullptr, SS_ERR_ARG, "ss_erase_table: bad argument");
    const ss_stream_erase e = erase ? *erase : ss_stream_erase{0, 0};
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) m += erase_keeps(regions[i], e.min_len_s) ? 1 : 0;
    *n_out = m;
    if (!out) return SS_OK;
    if (cap < m) return fail(nullptr, SS_ERR_CAPACITY, "ss_erase_table: capacity < " + std::to_string(m));
    m = 0;
    for (int64_t i = 0; i < n; ++i) if (erase_keeps(regions[i], e.min_len_s)) out[m++] = erase_padded(regions[i], e.pad_s);
    return SS_OK;
}

// The limit time L of include/softspoken.h, rounded as silence_ranges rounds a region's edge.  pending_start / pending_end are the walk's
// bin times (RunMerger::cur's, before the -3 s); the filter is evaluated on the values the table will hold.
extern "C" int64_t ss_stream_output_limit(int sr, int64_t bins_final, int pending, double pending_start, double pending_end,
                                          const ss_stream_erase* erase) {
    if (sr <= 0 || bins_final < 0 || !erase_ok(erase) || (pending && !(pending_end >= pending_start))) return INT64_MIN;
    const ss_stream_erase e = erase ? *erase : ss_stream_erase{0, 0};
    double L;
    if (!pending) L = (bin_time(bins_final) - 3.0) - e.pad_s;
    else {
        const ss_region r{pending_start - 3.0, pending_end - 3.0};
        L = erase_keeps(r, e.min_len_s) ? erase_padded(r, e.pad_s).end : erase_padded(r, e.pad_s).start;
    }
    const double f = std::nearbyint(L * (double)sr);
    return (int64_t)std::min(std::max(f, -9.0e18), 9.0e18);
}
static int64_t floor_div(int64_t a, int64_t b) { int64_t q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) --q; return q; }

// The separation streams' limit (include/softspoken.h "separation streams: the rule"): the smallest of the three conditions' first
// frames that may not be returned.  Condition 3 in integers: frame k reads the bins j0, j0 + 1 with j0 = floor((512 (k hop + 3 sr) - 3 sr) / (6 sr));
// j0 <= b - 2 <=> 512 k hop <= sr (6 b - 1539) - 1, and frame n needs frame floor(n / hop) + 2.
extern "C" int64_t ss_stream_separate_limit(int sr, int64_t frames_decoded, int64_t bins_final, int pending, double pending_start,
                                            double pending_end, const ss_stream_erase* erase, const ss_separation_params* params) {
    std::string err;
    if (sr <= 0 || sr > 768000 || frames_decoded < 0 || bins_final < 0 || bins_final > ((int64_t)1 << 40) || check_separation_params(params, err)) return INT64_MIN;
    const int64_t lz = ss_stream_output_limit(sr, bins_final, pending, pending_start, pending_end, erase);
    if (lz == INT64_MIN) return INT64_MIN;
    const ss_separation_params prm = params ? *params : separation_defaults();
    const int64_t F = (int64_t)std::nearbyint(prm.fade_s * (double)sr), N = sep_fft_size(sr), hop = N / 4;
    const int64_t c1 = std::min(std::max<int64_t>(lz, 0), frames_decoded) - F, c2 = frames_decoded - N;
    int64_t c3 = 0;
    if (bins_final >= 1) {
        const int64_t T = floor_div((int64_t)sr * (6 * bins_final - 1539) - 1, 512);
        c3 = (floor_div(T, hop) - 1) * hop;
    }
    return std::min(c1, std::min(c2, c3));
}

extern "C" double ss_stream_separate_latency(int sr, double break_s, const ss_stream_erase* erase, const ss_separation_params* params) {
    std::string err;
    if (sr <= 0 || sr > 768000 || !std::isfinite(break_s) || !erase_ok(erase) || check_separation_params(params, err)) return std::nan("");
    const ss_stream_erase e = erase ? *erase : ss_stream_erase{0, 0};
    const ss_separation_params prm = params ? *params : separation_defaults();
    const double half = sr == SS_SAMPLE_RATE ? 0.0 : std::ceil(32.0 / std::min(1.0, 22050.0 / (double)sr));
    const double B = 3.0 + 2.0 * (3.0 / 256.0) + half / (double)sr, D = B + std::max(break_s, 0.0) + e.pad_s + e.min_len_s;
    return D + prm.fade_s + (double)(sep_fft_size(sr) + 1) / (double)sr;
}

// Canonical 44-byte RIFF/WAVE header of a 16-bit PCM file (what libsndfile writes for subtype PCM_16).
extern "C" int ss_wav_header_pcm16(int sr, int ch, int64_t frames, void* out44) {
    const int64_t data = frames * ch * 2;
    if (!out44 || sr <= 0 || ch < 1 || ch > 64 || frames < 0 || data + 36 > 0xFFFFFFFFLL)
        return fail(nullptr, SS_ERR_ARG, "ss_wav_header_pcm16: bad argument (a RIFF file holds < 4 GiB)");
    unsigned char* h = (unsigned char*)out44;
    auto u32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; ++i) h[at + i] = (unsigned char)(v >> (8 * i)); };
    auto u16 = [&](int at, uint32_t v) { h[at] = (unsigned char)v; h[at + 1] = (unsigned char)(v >> 8); };
    memcpy(h, "RIFF", 4); u32(4, (uint32_t)(36 + data)); memcpy(h + 8, "WAVEfmt ", 8); u32(16, 16);
    u16(20, 1); u16(22, (uint32_t)ch); u32(24, (uint32_t)sr); u32(28, (uint32_t)(sr * ch * 2)); u16(32, (uint32_t)(ch * 2)); u16(34, 16);
    memcpy(h + 36, "data", 4); u32(40, (uint32_t)data);
    return SS_OK;
}

// The same 44 bytes for any of the little-endian encodings 1-6: format tag 1 (PCM) or 3 (IEEE float), the sample's own width.  For
// SS_PCM_S16 these are ss_wav_header_pcm16's bytes.  The big-endian encodings 7-12 have no RIFF/WAVE form.
extern "C" int ss_wav_header(int format, int sr, int ch, int64_t frames, void* out44) {
    if (!out44 || format < SS_PCM_U8 || format > SS_PCM_F64 || sr <= 0 || ch < 1 || ch > 64 || frames < 0 || frames > ((int64_t)1 << 36))
        return fail(nullptr, SS_ERR_ARG, "ss_wav_header: bad argument (encodings 1-6 only)");
    const int64_t bps = (int64_t)pcm_bytes_per_sample(format), data = frames * ch * bps;
    if (data + 36 > 0xFFFFFFFFLL) return fail(nullptr, SS_ERR_ARG, "ss_wav_header: bad argument (a RIFF file holds < 4 GiB)");
    unsigned char* h = (unsigned char*)out44;
    auto u32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; ++i) h[at + i] = (unsigned char)(v >> (8 * i)); };
    auto u16 = [&](int at, uint32_t v) { h[at] = (unsigned char)v; h[at + 1] = (unsigned char)(v >> 8); };
    memcpy(h, "RIFF", 4); u32(4, (uint32_t)(36 + data)); memcpy(h + 8, "WAVEfmt ", 8); u32(16, 16);
    u16(20, format >= SS_PCM_F32 ? 3 : 1); u16(22, (uint32_t)ch); u32(24, (uint32_t)sr); u32(28, (uint32_t)((int64_t)sr * ch * bps));
    u16(32, (uint32_t)(ch * bps)); u16(34, (uint32_t)(8 * bps));
    memcpy(h + 36, "data", 4); u32(40, (uint32_t)data);
    return SS_OK;
}
