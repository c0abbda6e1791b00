/*
 * softspoken.h -- C ABI of libsoftspoken_hip.so: the MI355X (gfx950) implementation of Softspoken's
 * "Run Voice Detector" hot path.  Plain pointers and sizes only; no torch / numpy types.
 *
 * The reference (AVianEco/Softspoken) has no FFI: its boundary is a Python surface.  Each entry
 * point below names the reference code it stands behind (paths relative to the reference root):
 *
 *   ss_wav_parse, ss_resampled_length      root/code/backend/voice_activity.py:23-30   get_audio_data
 *   ss_plan_windows / ss_plan_windows_step root/code/frontend/NNDetector.py:55-82      plan_detection_job
 *   ss_window_start_bin,                   NNDetector.py:69,175 + root/code/backend/settings.py:16   settings.step_size
 *   ss_set_window_step / ss_get_window_step
 *   ss_create / ss_destroy                 NNDetector.py:21-34,42-53                   model build + load_checkpoint
 *   ss_upload_wav_batch_async              root/code/backend/worker.py:57 -> voice_activity.py:37 (sf.read of every file of the job)
 *   ss_add_pcm / ss_add_pcm_device /       voice_activity.py:32-69 load_audio  +  root/code/backend/worker.py:58-62 (3 s pad)
 *   ss_add_pcm_batch_device /
 *   ss_add_f32_22k / ss_add_padded_f32_22k
 *   ss_read_signal                         (returns what load_audio returns: float32 @ 22050 Hz)
 *   ss_features                            root/code/backend/pytorch_neural_nets.py:92-99,144-153 (mel front-end)
 *   ss_infer_windows                       NNDetector.py:84-101 process_batch -> SpecUNet_2D.forward (pytorch_neural_nets.py:142-197)
 *   ss_run (ss_run_begin + ss_run_end)     worker.py:49-100 (per-file loop: batches, averaging, regions, -3 s)
 *   ss_get_avg                             NNDetector.py:153-190 average_overlapping_detections
 *   ss_get_regions / ss_find_regions       NNDetector.py:103-143 find_speech_regions + worker.py:100
 *   ss_format_csv_rows                     worker.py:103-125 + root/code/frontend/silencer_ui.py:816-817 (DataFrame.to_csv text)
 *   ss_separation_plan / _maps /           silencer_ui.py:974-998 (SilenceWorker.run) with the spec head the reference computes and drops:
 *   ss_separate_pcm (_channels)            pytorch_neural_nets.py:125-130,184-185 (spec_output_conv, "env / speech separation"),
 *                                          NNDetector.py:84-101 (process_batch's speech_pred), worker.py:78-79; averaging NNDetector.py:168-186
 *
 * Conventions: every function returns an int status (SS_OK == 0) unless stated; the caller owns all
 * host buffers passed in and they only need to stay alive for the duration of the call; the library
 * owns all device memory.  One context per GPU; a context is NOT thread-safe, different contexts
 * are independent.  Calls may come from any host thread (the reference calls from a QThreadPool
 * thread, silencer_ui.py:243).  Unlike the reference, decode / IO / device failures are reported,
 * never swallowed (voice_activity.py:39-41 returns (None, None) and the worker then crashes).
 */
#ifndef SOFTSPOKEN_H
#define SOFTSPOKEN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_ABI_VERSION 3   /* 2: ss_kernel_stat.name[128], SS_ERR_RANGE, ingest (ss_host_alloc, ss_upload_wav_batch_async, ...); 3: ss_kernel_stat.issued_flops */

/* fixed properties of the path (reference settings.py:4-16, NNDetector.py:69-75) */
#define SS_SAMPLE_RATE 22050
#define SS_WINDOW_SAMPLES 66150   /* 3 s */
#define SS_STEP_SAMPLES 13230     /* floor(22050 * 0.6): the sample step of the default window step (ss_set_window_step) */
#define SS_STEP_DEFAULT 0.6       /* settings.py:16 step_size, seconds */
#define SS_STEP_MIN 0.1           /* window steps a context accepts: SS_STEP_MIN <= step_s <= SS_STEP_MAX, finite */
#define SS_STEP_MAX 3.0
#define SS_N_MELS 128
#define SS_N_FRAMES 256           /* time bins per window */

typedef struct ss_ctx ss_ctx;

enum ss_status {
    SS_OK = 0,
    SS_ERR_ARG = 1,      /* bad argument */
    SS_ERR_HIP = 2,      /* HIP runtime / kernel failure (message has the HIP error string) */
    SS_ERR_FORMAT = 3,   /* malformed weights blob or WAV */
    SS_ERR_STATE = 4,    /* call out of order (e.g. ss_run before any ss_add_*) */
    SS_ERR_STOPPED = 5,  /* stop flag observed; partial results of the current run are discarded */
    SS_ERR_NOMEM = 6,
    SS_ERR_CAPACITY = 7, /* caller's output buffer too small; required size is reported */
    SS_ERR_RANGE = 8     /* SS_FLAG_F16X2 only: a weight or an activation left the f16 range (|x| > 65504 after the build's power-of-two
                            channel normalisation) or was not finite; the results of the call are not to be used -- run this checkpoint
                            in the fp32 mode (flags without a precision bit).  The drop-in does that by itself (NNDetector.detect_files) */
};

enum ss_pcm_format {     /* sample encodings, interleaved: 1-6 = the WAV data chunk's (little endian); 7-12 = the AIFF / AIFF-C sound chunk's
                          * (big endian, 8-bit samples signed), round 4: libsndfile, which the reference reads files with
                          * (voice_activity.py:37), converts all of them to float the same way, x / 2^(bits-1) */
    SS_PCM_U8 = 1, SS_PCM_S16 = 2, SS_PCM_S24 = 3, SS_PCM_S32 = 4, SS_PCM_F32 = 5, SS_PCM_F64 = 6,
    SS_PCM_S8 = 7, SS_PCM_S16BE = 8, SS_PCM_S24BE = 9, SS_PCM_S32BE = 10, SS_PCM_F32BE = 11, SS_PCM_F64BE = 12
};

enum ss_flags {
    SS_FLAG_BF16 = 1u,       /* conv stack in bf16 with fp32 accumulation (throughput mode: scores differ from the reference by up to ~0.1) */
    SS_FLAG_PROFILE = 2u,    /* time every kernel launch with HIP events (ss_get_kernel_stats) */
    SS_FLAG_F16X2 = 4u       /* conv stack on the f16 matrix cores with every fp32 operand split into two f16 halves (x = hi + lo; three
                                products per term: w_hi x_hi + w_hi x_lo + w_lo x_hi, fp32 accumulation): scores within 1e-4 of the
                                reference's fp32 like the default, at 2.8 x its speed.  Every tensor is kept near 1 by an exact power-of-two
                                channel normalisation chosen from the weights at ss_create, so a checkpoint's BatchNorm gains do not decide
                                whether it fits; a value that still has no f16 representation (not finite, or beyond 65504 in normalised
                                units) is reported as SS_ERR_RANGE.  Default (no precision flag): fp32 operands on the fp32 matrix
                                instructions, an exact fp32 FMA chain */
};

typedef struct ss_wav_info {
    int32_t format;        /* enum ss_pcm_format */
    int32_t channels;
    int32_t sample_rate;
    int32_t bits;
    int64_t frames;
    int64_t data_offset;   /* byte offset of the first sample in the file */
    int64_t data_bytes;
} ss_wav_info;

typedef struct ss_region {  /* seconds relative to the start of the file (the reference's "-3" already applied) */
    double start;
    double end;
} ss_region;

typedef struct ss_kernel_stat {
    char name[128];        /* "<kernel instantiation as rocprofv3 prints it>/<layer>" */
    int64_t launches;
    double total_ms;        /* sum of HIP-event durations (SS_FLAG_PROFILE only) */
    double flops;           /* algorithmic FLOPs summed over launches (0 for byte-bound kernels) */
    double bytes;           /* algorithmic bytes summed over launches */
    double issued_flops;    /* FLOPs the matrix pipe was actually given: 2 x (products issued per multiply-add: 3 in f16x2, 1 otherwise) x the
                             * multiply-adds of the form that ran (the sub-pixel launches run 4 taps instead of 9 on their upsampled half) */
} ss_kernel_stat;

/* progress callback: done/total windows of the current run, called on the calling thread with the reference's sequence of values
 * -- done = 32, 64, ... (settings.prediction_batch_size; it emits after each batch, worker.py:82-84), then the total --.  The
 * passes through the network keep their full size (ss_set_chunk_windows): the values that fall into a pass are reported, in
 * order, when that pass has completed on the device. */
typedef void (*ss_progress_fn)(void* user, int64_t windows_done, int64_t windows_total);

/* ---- host-only helpers (no GPU needed) ----------------------------------------------------- */
int ss_abi_version(void);
/* last error message of the calling thread for calls that have no context (or ctx == NULL) */
const char* ss_last_error(const ss_ctx* ctx);

/* Walk a RIFF/WAVE image (PCM 8/16/24/32, IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE) or, since round 4, an AIFF / AIFF-C one ("FORM",
 * COMM + SSND chunks; big-endian PCM 8/16/24/32, AIFF-C "NONE" / "sowt" (little-endian PCM) / "fl32" / "fl64"): the containers
 * soundfile.read hands the reference as float32 (voice_activity.py:37).  Other containers (FLAC, OGG) are reported as SS_ERR_FORMAT. */
int ss_wav_parse(const void* file_bytes, size_t nbytes, ss_wav_info* out);
/* ceil(frames * 22050 / sample_rate): length of the resampled signal (librosa.resample's rule). */
int64_t ss_resampled_length(int64_t frames, int sample_rate);
/* Window start table of one file.  Returns the number of windows W (also when starts == NULL);
 * writes min(W, cap) entries.  starts[i] = i * 13230 into the 3 s-padded signal. */
int64_t ss_plan_windows(double duration_s, int64_t* starts, int64_t cap);
/* The same for a window step of step_s seconds (settings.step_size, NNDetector.py:69-78): per_step = floor(22050.0 * step_s),
 * W = ceil((round(duration_s * 22050) + 6 * 22050 - 66150) / per_step), starts[i] = i * per_step.  ss_plan_windows(d, ...) is
 * ss_plan_windows_step(d, 0.6, ...).  Returns -1 for a step outside [SS_STEP_MIN, SS_STEP_MAX] or not finite. */
int64_t ss_plan_windows_step(double duration_s, double step_s, int64_t* starts, int64_t cap);
/* First averaged bin of window i (NNDetector.py:175): int(round(i * step_size / (3 / 256))) as Python evaluates it -- the double
 * product, the double quotient, then the nearest integer with ties to even (99 / 512 s gives 16.5 i: 16, 33, 50, 66, 82).  The sample
 * step is floored and the bin step is not, so the two drift apart where 22050 * step_s is no integer (99 / 512 s: 0.48 s per hour of
 * audio); that is the reference's arithmetic and it is reproduced, not corrected.  Returns -1 for a bad step or i < 0. */
int64_t ss_window_start_bin(int64_t i, double step_s);
/* Threshold + run-length + gap merge on averaged logits (double), exactly as the reference does it
 * through "%.4f" time strings; bin_idx[i] is the bin number of avg[i].  Returns regions in seconds
 * minus 3.  *n_out receives the number found; SS_ERR_CAPACITY if it exceeds cap. */
int ss_find_regions(const double* avg, const int64_t* bin_idx, int64_t n, double threshold, double break_s,
                    ss_region* out, int64_t cap, int64_t* n_out);
/* The merged table of a recording whose channels were run alone ("speech on any channel"): avg holds n_channels series of n bins
 * each, channel after channel, over the same bin_idx.  A bin is above when any channel's value is > threshold (a NaN is not above and
 * does not hide the other channels); everything else is ss_find_regions -- the result is ss_find_regions on the element-wise,
 * NaN-ignoring maximum (fmax) of the channels, and n_channels == 1 is ss_find_regions itself.  SS_ERR_ARG for n_channels < 1. */
int ss_find_regions_union(const double* avg, const int64_t* bin_idx, int64_t n, int n_channels, double threshold, double break_s,
                          ss_region* out, int64_t cap, int64_t* n_out);
/* CSV body lines (no header) for `n` regions of one file, first ID = first_id, DataFrame.to_csv text.
 * Returns bytes needed (excluding NUL); writes at most cap bytes. */
int64_t ss_format_csv_rows(const char* file_path, const char* file_name, const ss_region* regions, int64_t n,
                           int64_t first_id, char* out, int64_t cap);

/* ---- context -------------------------------------------------------------------------------- */
/* weights_blob == NULL creates an audio-only context (ss_add_pcm / ss_read_signal work, model calls
 * return SS_ERR_STATE).  weights_blob: "SSWBLOB1" container of the checkpoint's state_dict tensors (packed by
 * softspoken_amd.checkpoint.pack_state_dict).  BatchNorm folding and MFMA fragment packing happen here. */
int ss_create(int device_id, const void* weights_blob, size_t nbytes, uint32_t flags, ss_ctx** out);
void ss_destroy(ss_ctx* ctx);
/* windows processed per pass through the conv stack (activation workspace is sized for this) */
int ss_set_chunk_windows(ss_ctx* ctx, int chunk);
/* The window step of the context, seconds (settings.step_size; default SS_STEP_DEFAULT): ss_run, ss_run_begin*, ss_run_from_logits and
 * the streams opened from now on plan with ss_plan_windows_step(duration, step_s) and average window i from bin
 * ss_window_start_bin(i, step_s).  Accepted: SS_STEP_MIN <= step_s <= SS_STEP_MAX, finite -- inside that range every bin up to the last
 * window's end has a window and at most 31 windows cover a bin; above 3 s bins between windows would have none; anything else is
 * SS_ERR_ARG.  SS_ERR_STATE while a run is in flight.  The last ended run's results and getters are untouched, and a stream keeps the
 * step it was opened with (or its image's, ss_stream_import).  With the default step every result is bit for bit what it was before
 * the step could be set.  NOT following the step: ss_infer_windows and ss_features take explicit starts, and the separation silencer
 * (ss_separation_plan / ss_separation_maps / ss_separate_pcm) stays on 0.6 s whatever the context's step -- its output is defined
 * independently of detection settings, so that two users get the same bytes. */
int ss_set_window_step(ss_ctx* ctx, double step_s);
double ss_get_window_step(ss_ctx* ctx);   /* -1 for a NULL context */

/* ---- signal arena: files of the current job, resident in HBM ------------------------------- */
int ss_reset(ss_ctx* ctx);
/* counts the ss_reset calls of this context: a caller that caches file ids compares it to know whether they still name its files */
uint64_t ss_reset_generation(ss_ctx* ctx);
/* Decode + mixdown + resample + 3 s pad on the device.  pcm: interleaved samples (host memory). */
int ss_add_pcm(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames, int* file_id);
/* Same, but `pcm_dev` already is device memory of this GPU (bench: inputs resident in HBM). */
int ss_add_pcm_device(ss_ctx* ctx, const void* pcm_dev, int format, int sample_rate, int channels, int64_t frames,
                      int* file_id);
/* `n_files` recordings of one format stored back to back in one device buffer: decode + resample for
 * the whole batch in two launches.  File ids are first_file_id .. first_file_id + n_files - 1. */
int ss_add_pcm_batch_device(ss_ctx* ctx, const void* pcm_dev, int format, int sample_rate, int channels,
                            const int64_t* frames, int n_files, int* first_file_id);
/* Per-channel ingest: no mixdown.  A recording of `channels` channels becomes `channels` signals with consecutive file ids
 * *first_file_id + c, in channel order; signal c is bit for bit what ss_add_pcm stores for the one-channel PCM made of channel c's
 * samples (same format, rate and frames; same 3 s of padding and header duration).  The interleaved PCM is read once per two channels
 * by the resampler (once in all for 22 050 Hz input).  Afterwards the signals are ordinary files of the job.  Argument limits of
 * ss_add_pcm; channels == 1 is ss_add_pcm.  pcm: host memory; pcm_dev: device memory of this GPU, aligned to the size of a sample
 * (16-bit stereo is read as 32-bit words: 4 bytes, as for ss_add_pcm_device).  On an error the job keeps the files it had. */
int ss_add_pcm_channels(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames, int* first_file_id);
int ss_add_pcm_channels_device(ss_ctx* ctx, const void* pcm_dev, int format, int sample_rate, int channels, int64_t frames,
                               int* first_file_id);
/* `n_files` recordings back to back in one device buffer, as ss_add_pcm_batch_device: recording r, channel c gets file id
 * *first_file_id + r * channels + c. */
int ss_add_pcm_channels_batch_device(ss_ctx* ctx, const void* pcm_dev, int format, int sample_rate, int channels,
                                     const int64_t* frames, int n_files, int* first_file_id);
/* A signal that already is mono float32 at 22 050 Hz (the parity boundary). Pads 3 s each side. */
int ss_add_f32_22k(ss_ctx* ctx, const float* samples, int64_t n, int* file_id);
/* A signal stored as is, no padding added (what worker.py hands to process_batch; also any buffer of
 * back-to-back windows).  Its header duration is taken as (n - 6 s) / 22050, clamped at 0. */
int ss_add_padded_f32_22k(ss_ctx* ctx, const float* padded, int64_t n, int* file_id);
int64_t ss_signal_length(ss_ctx* ctx, int file_id, int padded);
int ss_read_signal(ss_ctx* ctx, int file_id, int padded, int64_t offset, int64_t n, float* out);
/* Silencer (silencer_ui.py:974-998 SilenceWorker.run): decode the interleaved samples
 * to float32 as the loader does, zero frames [round(start*sr), round(end*sr)) of every region (Python
 * round, clamped to the file; regions may overlap, be unsorted or lie outside the file), and return
 * interleaved 16-bit PCM -- lrintf(x * 32767), no clipping: what the reference's sf.write(path, data, sr)
 * stores, soundfile's default WAV subtype being PCM_16.  `out` holds frames*channels int16.  Any context
 * will do (audio-only included). */
int ss_silence_pcm(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames,
                   const ss_region* regions, int64_t n_regions, int16_t* out);
/* Review-screen spectrogram (voice_activity.py:148-154 wav_to_spec): magnitude of the STFT with
 * n_fft = win_length = 512 (settings.py:4-6), hop 256, periodic Hann, centred frames over zero padding (librosa.stft's
 * defaults).  out is [257][frames] float32, frames = ss_stft512_frames(n) = 1 + n / 256.  Any context will do. */
int64_t ss_stft512_frames(int64_t n_samples);
int ss_stft512_magnitude(ss_ctx* ctx, const float* samples, int64_t n_samples, float* out, int64_t cap_frames);
/* The 44-byte RIFF/WAVE header that goes in front of ss_silence_pcm's output.  Host only. */
int ss_wav_header_pcm16(int sample_rate, int channels, int64_t frames, void* out44);
/* device allocation helpers so a host without its own HIP binding can stage inputs in HBM (what is still allocated when the context
 * is destroyed is freed with it) */
int ss_device_alloc(ss_ctx* ctx, size_t nbytes, void** dev_ptr);
int ss_device_free(ss_ctx* ctx, void* dev_ptr);
int ss_device_upload(ss_ctx* ctx, void* dev_dst, const void* host_src, size_t nbytes);
/* ---- ingest: the job's WAV files from host memory into HBM, beside the kernels of the job before ----------------------
 * (worker.py:57 reads and decodes one file at a time in front of its batches; here the bytes of job k + 1 cross PCIe on the context's
 * copy stream while job k's kernels run on its compute stream.)
 * Page-locked host memory (hipHostMalloc): copies from it are asynchronous and run at the link's rate. */
int ss_host_alloc(ss_ctx* ctx, size_t nbytes, void** host_ptr);
int ss_host_free(ss_ctx* ctx, void* host_ptr);
/* n_files RIFF/WAVE images in host memory: the header walk of every file (ss_wav_parse -> infos[i]) and one asynchronous
 * host -> device copy per file of exactly frames * channels * bytes-per-sample bytes of its data chunk, back to back from
 * dev_dst (cap bytes; SS_ERR_CAPACITY when they do not fit), on the copy stream.  Returns when the copies are enqueued: the
 * file images must stay untouched until ss_upload_wait or the next ss_sync.  Allowed while a run is in flight (it touches
 * neither the signal arena nor the workspace).  A following ss_add_pcm_device / ss_add_pcm_batch_device on this context waits
 * for the copies ON THE DEVICE (an event between the two streams), not on the host.  The caller alternates two staging buffers:
 * the decode kernels of the job in flight read the other one. */
int ss_upload_wav_batch_async(ss_ctx* ctx, const void* const* files, const size_t* nbytes, int n_files, void* dev_dst, size_t cap,
                              ss_wav_info* infos);
/* the same for raw bytes (no header walk) */
int ss_device_upload_async(ss_ctx* ctx, void* dev_dst, const void* host_src, size_t nbytes);
/* host-side wait for every copy enqueued so far on the copy stream */
int ss_upload_wait(ss_ctx* ctx);

/* ---- compute -------------------------------------------------------------------------------- */
/* Mel front-end only: feat_out[n][128][256] float32 for windows starting at starts[i] (padded-signal index).
 * feat_out == NULL runs the kernels and discards the result (front-end timing). */
int ss_features(ss_ctx* ctx, int file_id, const int64_t* starts, int n, float* feat_out);
/* process_batch: mask_out[n][256] raw logits; spec_out (nullable) [n][2][128][256]. Any n >= 1. */
int ss_infer_windows(ss_ctx* ctx, int file_id, const int64_t* starts, int n, float* mask_out, float* spec_out);
/* Whole job over every file added since ss_reset: plan windows from each file's header duration,
 * (ss_plan_windows_step with the context's window step, ss_set_window_step), front-end + conv stack over all windows in chunks
 * (across file boundaries), overlap averaging on the device, region finding on the host.  stop_flag (nullable) is polled between chunks. */
int ss_run(ss_ctx* ctx, double threshold, double break_s, ss_progress_fn progress, void* user,
           const volatile int* stop_flag);
/* The same job in two halves (worker.py:49-100 has no counterpart: its loop is synchronous).  ss_run_begin plans and enqueues
 * everything up to the last device -> host copy and returns; ss_run_end waits for it and finds the regions.  Between the two
 * the context accepts no ss_reset / ss_add_* / compute call (SS_ERR_STATE).  A caller with two contexts on one device alternates
 * them, so that one job's host half runs while the other job's kernels do: ss_run == ss_run_begin + ss_run_end. */
int ss_run_begin(ss_ctx* ctx, double threshold, double break_s);
int ss_run_end(ss_ctx* ctx);
/* ss_run_begin with an event behind every pass, and the progress of the run in flight read from them: ss_run_poll calls
 * `progress` with the values of ss_progress_fn's sequence that have completed since the last call -- block != 0: waits for all of
 * them --.  A caller that keeps the device busy with file k + 1 while it files the rows of file k reports k + 1's progress from
 * here when its turn comes (root/code/backend/worker.py).  ss_run(progress) == ss_run_begin_tracked + ss_run_poll(block) + ss_run_end. */
int ss_run_begin_tracked(ss_ctx* ctx, double threshold, double break_s);
int ss_run_poll(ss_ctx* ctx, ss_progress_fn progress, void* user, int block);
/* The tail of ss_run for files whose per-window logits were computed elsewhere -- a long recording whose window ranges ran on
 * several GPUs (windows are independent, NNDetector.py:55-82; averaging needs the neighbours, :168-186, so the
 * logits are gathered to the recording's owner): logits[n_windows][256] for every window of every file added since ss_reset, in
 * file order, as ss_get_window_logits returns them.  Averaging, thresholding and region finding are ss_run's own code, so the table
 * equals that of a one-GPU ss_run bit for bit.  Works on an audio-only context too.  n_windows must equal the plan's total. */
int ss_run_from_logits(ss_ctx* ctx, const float* logits, int64_t n_windows, double threshold, double break_s);
/* Results are those of the last ENDED run; file_id counts that run's files from 0.  The regions (ss_get_regions*, found when first
 * asked for) and ss_num_windows stay readable while the next job is added and in flight, so one context can also overlap the host
 * half of job k with the device half of job k + 1: ss_run_end(k), ss_reset, ss_add_*(k + 1), ss_run_begin(k + 1), then the getters
 * for k.  ss_get_window_logits / ss_get_avg read device buffers that the next ss_run_begin reuses: after it, or after ss_reset,
 * they return SS_ERR_STATE. */
int64_t ss_num_windows(ss_ctx* ctx, int file_id);
int ss_get_window_logits(ss_ctx* ctx, int file_id, float* out, int64_t cap_windows);   /* [W][256] */
/* averaged logits (double) and their bin numbers; returns count via *n_out */
int ss_get_avg(ss_ctx* ctx, int file_id, double* avg, int64_t* bin_idx, int64_t cap, int64_t* n_out);
int ss_get_regions(ss_ctx* ctx, int file_id, ss_region* out, int64_t cap, int64_t* n_out);
/* The same for files [first_file, first_file + n_files) in one call: counts[i] regions of file first_file + i, back to
 * back in out (either may be NULL; *n_out = total). */
int ss_get_regions_batch(ss_ctx* ctx, int first_file, int n_files, int64_t* counts, ss_region* out, int64_t cap, int64_t* n_out);
/* The merged table of files [first_file, first_file + n_channels) of the ended run -- the channels of one recording added with
 * ss_add_pcm_channels*: ss_find_regions_union of their averages with the run's threshold and break (found from the run's bin masks,
 * so it is readable as long as ss_get_regions is).  out may be NULL (*n_out = count).  SS_ERR_ARG when the range is not inside the
 * run or the files differ in their number of bins. */
int ss_get_regions_union(ss_ctx* ctx, int first_file, int n_channels, ss_region* out, int64_t cap, int64_t* n_out);
/* Which channel heard a merged region: peaks[r * n_channels + c] = the maximum of channel c's averaged score over the covered bins from
 * region r's first to its last bin, both included (NaNs passed over; -inf when every one is NaN).  Channel c heard region r when its
 * peak is > threshold; at least one did.  Computed on the device from the averages: valid as long as ss_get_avg is.  peaks may be
 * NULL (*n_out = number of merged regions); SS_ERR_CAPACITY when cap_regions is smaller. */
int ss_get_region_peaks(ss_ctx* ctx, int first_file, int n_channels, double* peaks, int64_t cap_regions, int64_t* n_out);

/* ---- streaming detection: one recording's PCM arriving in pieces, its final regions returned early -----------------------
 * A stream is one recording in one enum ss_pcm_format encoding, rate and channel count (the limits of ss_add_pcm), pushed in pieces
 * of any size down to one frame; its threshold, break and window step (the context's, ss_set_window_step) are fixed when it is opened.  Each step takes every stream of the context as
 * far as its pushed audio allows -- decode + mixdown (or, in each-channel mode below, one signal per channel) + resample with carried state, every window that has become complete (in passes
 * of up to ss_set_chunk_windows windows, mixed across streams), the averaging of the bins that became final, the regions -- and
 * returns what became final.  Equality: the concatenation of every region and every averaged bin a stream returned equals what
 * ss_add_pcm + ss_run(threshold, break_s) give for the same frames on a context of the same precision and window step (regions as ss_region values,
 * averages as doubles, bit for bit), for any split into pieces, any cadence of steps and whichever streams shared the passes.
 * Returned results are final (never changed or withdrawn).
 *
 * Latency bound B.  A bin at audio time t (seconds from the recording's start, bin_time - 3) is returned by the first step after the
 * stream holds audio past t + B, and a region whose last above-threshold bin lies at t_end by the first step after it holds audio
 * past t_end + break_s + B, where
 *     B = 3 s + 2 x (3 / 256) s + half / sample_rate,        half = ceil(32 / min(1, 22050 / sample_rate)) (0 at 22 050 Hz):
 * the last window over a bin ends at most 3 s of audio after it (plus half a bin of the rounded start, ss_window_start_bin; the sample
 * step is floored, so a window's audio never lies later than its nominal time i x step: B holds for every window step), the gap test
 * of a region needs one more bin past t_end + break_s (the 4-decimal rounding of bin times is below a bin), and a resampled sample
 * waits for `half` input frames after it.  16 kHz: 3.0254 s; 44.1 / 48 kHz: 3.0249 s; 8 kHz: 3.0274 s.  The bins and regions of
 * the last seconds are final at close, as in ss_run (the plan's window and bin counts depend on the total duration).
 *
 * State.  Between steps a stream holds the 22 050 Hz samples from its first window not yet run (< 3 s + step: 3.6 s at the default), its
 * resampler's input history (< 2 half + 1 frames), the logits of the <= ceil(256 / s_b) + 1 windows over its non-final bins (s_b =
 * step x 256 / 3 bins per window: 6 windows at the default, 31 at 0.1 s), its open region and counters: a size that does not grow with
 * the stream.  Pushed pieces wait in library-owned host staging until a step takes them.
 * Streams and the job calls share a context without touching each other: a step reads none of the files, results or getters of
 * the last ended run, ss_run / ss_reset leave the streams alone; a step while ss_run_begin is in flight is SS_ERR_STATE. */
typedef struct ss_stream_info {
    int64_t frames_pushed;     /* frames pushed so far (stepped and staged) */
    int64_t frames_staged;     /* of them: waiting for the next step */
    int64_t windows_run;       /* windows of the recording run so far -- per channel: an each-channel stream of C channels ran C x as many */
    int64_t windows_ready;     /* windows the next step would run, per channel likewise (> 0: the stream takes part in it) */
    double final_until_s;      /* audio time before which every bin is final (returned) */
    int32_t closed;            /* ss_stream_close was called */
    int32_t finished;          /* closed and the last step has run: every result is out */
    int64_t state_bytes;       /* bytes the stream carries between steps (device samples, logits, host record), staging excluded; an
                                  each-channel stream: every lane once, the raw PCM held for output once */
} ss_stream_info;

/* Open a stream; *stream_id names it on this context.  Needs a context with weights. */
int ss_stream_open(ss_ctx* ctx, int format, int sample_rate, int channels, double threshold, double break_s, int* stream_id);
/* Copy `frames` interleaved frames from host memory into the stream's staging (any number, 0 included).  Not after close. */
int ss_stream_push(ss_ctx* ctx, int stream_id, const void* pcm, int64_t frames);
/* End of input: the next step runs the windows that read the end padding, finalises the last bins and regions, and finishes it. */
int ss_stream_close(ss_ctx* ctx, int stream_id);
/* One step over every stream of the context (see above).  Each stream's results of the previous step are replaced by this
 * step's (empty when it had nothing new), so nothing accumulates when a caller does not read.  f16x2: a step whose passes set the
 * range flag returns SS_ERR_RANGE and commits nothing -- every stream is as it was before the step, its staged input kept
 * (ss_stream_export it into an fp32 context and step there). */
int ss_stream_step(ss_ctx* ctx);
/* The regions the last step finalised for the stream: seconds from the recording's start, the reference's -3 s applied, like
 * ss_get_regions.  *n_out = count; SS_ERR_CAPACITY when it exceeds cap (out may be NULL to ask for the count). */
int ss_stream_regions(ss_ctx* ctx, int stream_id, ss_region* out, int64_t cap, int64_t* n_out);
/* The averaged bins the last step finalised (covered bins only, ascending), with the bin numbers ss_get_avg gives them for the
 * whole recording.  Either pointer may be NULL. */
int ss_stream_avg(ss_ctx* ctx, int stream_id, double* avg, int64_t* bin_idx, int64_t cap, int64_t* n_out);
int ss_stream_get_info(ss_ctx* ctx, int stream_id, ss_stream_info* out);
/* Release a stream, at any time. */
int ss_stream_free(ss_ctx* ctx, int stream_id);
/* A stream's whole state (staging included, the last step's results excluded) as a byte image: *n_out = its size (buf may be NULL
 * to ask); SS_ERR_CAPACITY when cap is smaller.  ss_stream_import makes a new stream of another (or the same) context from it --
 * of any precision: what the f16x2 fallback and a feed that moves to another device need.  The image carries the stream's window
 * step (a stream with the default step writes the image it always wrote, "SSSTRM01"; any other step writes "SSSTRM02", the step appended
 * to the header); ss_stream_import reads both and the new stream keeps the image's step whatever the context's. */
int ss_stream_export(ss_ctx* ctx, int stream_id, void* buf, int64_t cap, int64_t* n_out);
int ss_stream_import(ss_ctx* ctx, const void* buf, int64_t n, int* stream_id);

/* ---- streaming silencer: a stream's frames back as final 16-bit PCM, the detected speech zeroed ------------------------------
 * A stream opened with ss_stream_open_output also returns, after every step, the next run of the recording's frames as interleaved
 * 16-bit PCM (ss_stream_output).  Returned frames are final and contiguous: every step continues where the last one ended.
 * Equality: the concatenation of everything ss_stream_output returned from open until the stream finished equals, byte for byte,
 *     ss_silence_pcm(the whole recording, E(R)),    R = the concatenation of the regions the same stream returned,
 * for any split into pieces, any cadence of steps, whichever streams shared the step, and across ss_stream_export / _import.
 *
 * Erase table E(R; pad_s, min_len_s) (ss_erase_table): every region with end - start <= min_len_s is dropped (the review screen's
 * filter, on the table's doubles), every other one becomes [start - pad_s, end + pad_s]; ss_silence_pcm then rounds, clamps and merges
 * as it always does.  Both parameters are finite and >= 0; NULL means 0, 0.  (A voice starts before its score crosses the threshold:
 * pad_s; nobody reviews a live feed: min_len_s.)
 *
 * Which frames a step returns.  A frame is decided when its output value is the same for every continuation of the recording.  With b
 * final bins and P the merged candidate that is not final yet (the walk's current region, joined with the open run of bins above the
 * threshold when that run starts within break_s of its end), the limit time is
 *     no P:                              L = (bin_time(b) - 3) - pad_s       (no later region can start earlier)
 *     P already passes the filter:       L = (P.end - 3) + pad_s             (P only grows: up to there it is erased whatever follows)
 *     P does not pass the filter yet:    L = (P.start - 3) - pad_s
 * and the step returns the frames [frames_out, min(max(nearbyint(L x sample_rate), frames_out), frames decoded)); at close, all of
 * them (ss_stream_output_limit is this rule, host only).  A current region that an open run can no longer reach (the run started more
 * than break_s behind its end) is final though not returned yet, and is erased as such.
 *
 * Latency bound D.  A frame at audio time t is returned by the first step after the stream holds audio past t + D,
 *     D = B + break_s + pad_s + min_len_s         (B: the bound of the bins above).
 * Derivation: with audio held up to H every bin before H - B + (3 / 256) s is final (B carries one bin more than a bin needs), so
 * bin_time(b) - 3 >= H - B + 3 / 256.  An open run ends at bin b - 1; a current region without an open run ends at most break_s before
 * bin b - 1 (or the walk had returned it); a P that fails the filter is at most min_len_s long.  So in every case
 * L >= bin_time(b - 1) - 3 - break_s - min_len_s - pad_s >= H - D.  (Bins no window covers neither open nor close a run; a whole-file
 * plan has them only behind the last window, where the close decides.)
 *
 * State.  A stream with output also carries its raw PCM from the first frame not returned to the last one decoded, on the device, in
 * its own encoding: at most D seconds plus what one step decoded, whatever the stream's length; ss_stream_info.state_bytes counts it.
 * A refused f16x2 step (SS_ERR_RANGE) commits nothing of the output either. */
typedef struct ss_stream_erase { double pad_s, min_len_s; } ss_stream_erase;
typedef struct ss_stream_output_info {
    int64_t frames_out;        /* frames returned so far: the next step's first_frame */
    int64_t frames_held;       /* frames pushed and not returned yet (carried on the device, or staged) */
    int64_t frames_erased;     /* of the frames returned: zeroed */
    double pad_s, min_len_s;   /* the stream's erase parameters */
} ss_stream_output_info;
/* E(R) as regions (host only): *n_out = count, SS_ERR_CAPACITY when it exceeds cap (out may be NULL to ask for the count).  Rows that
 * hold a NaN stay (ss_silence_pcm passes over them). */
int ss_erase_table(const ss_region* regions, int64_t n, const ss_stream_erase* erase, ss_region* out, int64_t cap, int64_t* n_out);
/* The limit frame nearbyint(L x sample_rate) of the rule above, before the clamp to [frames_out, frames decoded] (host only).
 * pending != 0: P exists; pending_start / pending_end are the bin times of its first and last bin BEFORE the reference's -3 s (the
 * filter is evaluated on (end - 3) - (start - 3), the values the table will hold).  INT64_MIN on a bad argument. */
int64_t ss_stream_output_limit(int sample_rate, int64_t bins_final, int pending, double pending_start, double pending_end,
                               const ss_stream_erase* erase);
/* ss_stream_open with output; erase == NULL: pad_s = min_len_s = 0.  The threshold may be infinite here (+inf: the plain transcode;
 * -inf: every bin a window covers is speech).  Everything else of the stream is ss_stream_open's. */
int ss_stream_open_output(ss_ctx* ctx, int format, int sample_rate, int channels, double threshold, double break_s,
                          const ss_stream_erase* erase, int* stream_id);
/* The frames the last step returned: frames [*first_frame, *first_frame + *n_frames) of the recording as *n_frames x channels int16.
 * out == NULL asks for the two counts; SS_ERR_CAPACITY when cap_frames < *n_frames; SS_ERR_STATE on a stream opened without output. */
int ss_stream_output(ss_ctx* ctx, int stream_id, int16_t* out, int64_t cap_frames, int64_t* first_frame, int64_t* n_frames);
int ss_stream_get_output_info(ss_ctx* ctx, int stream_id, ss_stream_output_info* out);
/* Images: a stream with output exports "SSSTRM03" (the header, the step, the erase parameters, frames_out, the decided ranges still
 * ahead and the held PCM); ss_stream_import reads all three, and a stream without output writes the image it always wrote. */

/* ---- each-channel streams: every channel detected alone, one merged table ------------------------------------------------------
 * ss_stream_open_channels opens a stream of C channels that carries C lanes, one per channel, instead of the one lane of the channel
 * mean: what ss_add_pcm_channels is to ss_add_pcm.  The lanes share the stream's plan (frame count, resampler positions, window and bin
 * counts, the frontier of final bins) and every ss_stream_* call works on such a stream.  For any split into pieces, any cadence of
 * steps, whichever other streams share the steps (mix streams included) and across ss_stream_export / ss_stream_import, on a context
 * of precision P and window step s:
 *   Per channel.    The concatenation of what ss_stream_avg_channel(stream, c) returned equals ss_get_avg(first_file + c) after
 *                   ss_add_pcm_channels + ss_run(threshold, break_s) of the same frames on a context of P and s: averages as doubles, bit
 *                   for bit, bin numbers exactly.
 *   Merged table.   The concatenation of ss_stream_regions equals ss_get_regions_union(first_file, C) of that run, as ss_region values.
 *   Merged series.  ss_stream_avg returns the series the table is found on: per covered bin the fmax over the channels' averages (a NaN
 *                   on one channel is passed over; NaN only when every channel's is), so ss_find_regions(ss_stream_avg ...) gives the
 *                   stream's regions, as for a mix stream.
 *   Peaks.          ss_stream_region_peaks returns peaks[r * C + c] for the regions the last step returned: the values
 *                   ss_get_region_peaks gives for the same regions of the whole-file run -- the fmax of channel c's averages over the
 *                   covered bins from the region's first to its last bin, both and the below-threshold bins of the gaps that break_s
 *                   merged included; -inf when all of them are NaN.  Bit for bit.
 *   Output.         With output, the concatenation of ss_stream_output equals ss_silence_pcm(the whole recording, E(R)), byte for byte,
 *                   R = the merged regions the stream returned: every channel is zeroed over the merged table.
 *   Bounds.         B, D and the limit rule ss_stream_output_limit hold unchanged; the walk that feeds them runs over the merged flags.
 *   One channel.    A one-channel recording opened here is a plain stream: the same path, results and image as ss_stream_open's (and
 *                   ss_stream_region_peaks answers SS_ERR_STATE, as on a mix stream).
 * erase == NULL and with_output == 0: detection only; otherwise a stream with output (erase == NULL: pad_s = min_len_s = 0), with
 * ss_stream_open_output's rule for the threshold. */
int ss_stream_open_channels(ss_ctx* ctx, int format, int sample_rate, int channels, double threshold, double break_s,
                            const ss_stream_erase* erase, int with_output, int* stream_id);
/* ss_stream_avg of one channel's lane (the same bins as ss_stream_avg's).  SS_ERR_ARG for a channel out of range; on a mix stream
 * channel 0 is ss_stream_avg itself. */
int ss_stream_avg_channel(ss_ctx* ctx, int stream_id, int channel, double* avg, int64_t* bin_idx, int64_t cap, int64_t* n_out);
/* *n_out = the regions the last step returned; peaks (NULL to ask) takes *n_out x channels doubles; SS_ERR_CAPACITY when cap_regions
 * is smaller; SS_ERR_STATE on a mix stream. */
int ss_stream_region_peaks(ss_ctx* ctx, int stream_id, double* peaks, int64_t cap_regions, int64_t* n_out);
/* Images: an each-channel stream of more than one channel exports "SSSTRM04" (the header, the step, the lane count, the peak state, the
 * output block of "SSSTRM03" when it has output, every lane's carried data), so the mode survives the move to an fp32 context;
 * ss_stream_import reads all four, and answers SS_ERR_ARG to an "SSSTRM04" image whose lane count is neither 1 nor its channel count
 * or whose sizes do not add up to n. */

/* ---- separation silencer: remove the speech part of the spectrum inside the erased intervals ---------------------------
 * The second silencing method.  ss_silence_pcm zeroes every reviewed interval (silencer_ui.py:974-998), and with it whatever
 * environmental sound overlaps the voice.  This one rebuilds the audio inside the same intervals from an STFT at the file's native
 * rate with the speech part removed.  The mask is a per-band gain from the network's second head, spec_output_conv
 * (pytorch_neural_nets.py:125-130,184-185: "env / speech separation", a ReLU'd (2, 128, 256) map per window that process_batch
 * returns as speech_pred, NNDetector.py:84-101, and worker.py:78-79 drops).  Outside the intervals the output is bit for bit
 * ss_silence_pcm's.  Definition, step by step:
 *  1. Windows and bins follow the detector at its default window step of 0.6 s (whatever ss_set_window_step says: two users get the same
 *     bytes): ss_plan_windows' windows over the ss_add_pcm signal, window i covers the bins
 *     round(51.2 i) .. + 255 (NNDetector.py:168-186), bin j is centred at (j + 0.5) 3 / 256 - 3 s (the reference's 3 / 256 s bin;
 *     the true hop is 256 / 22050 s).  The spec head runs on every window that covers a needed bin (step 3) and on no other.
 *     Each needed bin averages both channels over the windows that cover it: a float64 sum in ascending window order divided by
 *     the count, stored as float32 -- equal to a whole-file average bit for bit.
 *  2. Band gains: P_c = 10^(y_c^2) - 1 (inverse of the front-end's sqrt(log10(x + 1))), G = P_env / (P_env + P_speech) evaluated as
 *     a logistic of the log-power difference (finite for any finite y), G = 1 where both are 0, G' = max(G, min_gain).
 *  3. STFT at the native rate: N = 2^round(log2(sr 512 / 22050)) clamped to [256, 8192], hop N / 4, periodic Hann analysis and
 *     synthesis windows, overlap-add divided by sum w^2 = 1.5; frame k is centred on sample k hop (its support
 *     [k hop - N/2, k hop + N/2), samples outside the file are zeros).  Only frames whose support meets a merged interval run.
 *     STFT bin f = q sr / N Hz of frame k gets sum_m T_m(f) G'_m / sum_m T_m(f), T_m the front-end's HTK triangles (0 .. 8000 Hz,
 *     128 bands, no norm), band 0's gain at f = 0, 1 (SS_ABOVE_FMAX_KEEP) or min_gain (SS_ABOVE_FMAX_MUTE) at f >= 8000 Hz;
 *     in time, linear between the two bin centres around k hop / sr, clamped to the first / last bin that has a window.
 *     Every channel has its own STFT; all share the gain map of the mono mix the model sees.  The overlap-add is a gather in
 *     fixed frame order: two calls give identical bytes.
 *  4. Inside a merged interval [a, b): y = x + w (p - x), x the decoded sample, p the resynthesis, w a raised-cosine ramp
 *     w(d) = (1 - cos(pi (d + 0.5) / F)) / 2 over the F = round(fade_s sr) samples at each end (d = n - a at the start, b - 1 - n at
 *     the end, the smaller of the two), 1 in between.  Encoded as ss_silence_pcm encodes: lrintf(y * 32767), no clipping.
 * With min_gain 0, SS_ABOVE_FMAX_MUTE, fade_s 0 and a network whose speech map dominates everywhere, the output is ss_silence_pcm's. */
#define SS_ABOVE_FMAX_MUTE 0   /* STFT bins at or above 8000 Hz (the model's f_max) get min_gain */
#define SS_ABOVE_FMAX_KEEP 1   /* ... or pass unchanged */

typedef struct ss_separation_params {
    double fade_s;            /* >= 0; default 0.01 */
    double min_gain;          /* in [0, 1]; default 0 */
    int32_t above_fmax;       /* SS_ABOVE_FMAX_MUTE (default) or SS_ABOVE_FMAX_KEEP */
    int32_t speech_channel;   /* channel of the spec head that holds speech: 0 or 1; default 1 (the reference's "env / speech" order;
                                 the checkpoint itself is not at hand to confirm it) */
} ss_separation_params;       /* NULL params: the defaults */

typedef struct ss_separation_range {   /* one merged interval (silence_ranges' merge and rounding, as ss_silence_pcm) */
    int64_t frame_begin, frame_end;    /* [a, b) in frames of the file */
    int64_t stft_first, stft_last;     /* STFT frames k (inclusive) whose support meets [a, b); k may be negative */
    int64_t bin_first, bin_last;       /* averaged bins (inclusive) their gains read */
    int64_t win_first, win_last;       /* windows (inclusive) that cover any of those bins */
} ss_separation_range;

typedef struct ss_separation_plan_info {
    int32_t n_fft, hop;                /* N and N / 4 */
    int64_t n_windows;                 /* windows of the whole file (ss_plan_windows, clamped to the resampled signal as ss_run does) */
    int64_t n_bins;                    /* bins 0 .. n_bins - 1 have a window (the whole-file average's covered bins) */
    int64_t windows_run;               /* windows the spec head runs on: the union of the ranges' window ranges */
    int64_t n_ranges;                  /* out: merged intervals */
    int64_t cap_ranges;                /* in: entries `ranges` holds; SS_ERR_CAPACITY (n_ranges still set) when too few */
    ss_separation_range* ranges;       /* in: caller's array (NULL when cap_ranges == 0) */
} ss_separation_plan_info;

/* Host only: the plan of ss_separate_pcm for a file of `frames` frames at sample_rate (the limits of ss_add_pcm).  SS_ERR_ARG for
 * bad parameters: speech_channel not 0 / 1, fade_s < 0 or not finite, min_gain outside [0, 1], an unknown above_fmax. */
int ss_separation_plan(int sample_rate, int64_t frames, const ss_region* regions, int64_t n_regions, const ss_separation_params* params,
                       ss_separation_plan_info* out);
/* Averaged spec-head maps (step 1) of bins [first_bin, first_bin + n_bins) of a file already added: out[2][n_bins][128] float32,
 * channel-major as the head emits them.  Runs the spec head on exactly the windows that cover these bins (passes of
 * ss_set_chunk_windows).  SS_ERR_ARG when a bin has no window; SS_ERR_RANGE under SS_FLAG_F16X2 as ss_infer_windows. */
int ss_separation_maps(ss_ctx* ctx, int file_id, int64_t first_bin, int64_t n_bins, float* out);
/* The separation silencer (above): interleaved PCM in (any enum ss_pcm_format, rate and channel count ss_add_pcm takes), interleaved
 * 16-bit PCM out (frames * channels int16, as ss_silence_pcm).  Needs a context with weights (SS_ERR_STATE on an audio-only one or
 * while a run is in flight).  It acts as ss_reset + ss_add_pcm of this file -- ss_reset_generation counts it, earlier file ids and
 * the last run's results are gone --; streams are untouched.  SS_ERR_RANGE under SS_FLAG_F16X2 when the spec head's passes leave the
 * f16 range (run the file in an fp32 context), with `out` not to be used. */
int ss_separate_pcm(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames, const ss_region* regions,
                    int64_t n_regions, const ss_separation_params* params, int16_t* out);
/* Per-channel separation: the separation silencer for a recording detected with ss_add_pcm_channels* -- each channel's gains come from
 * its own network passes, not from the mono mix (which holds a voice that reached one microphone at half level, and cuts bands out of
 * the channels that did not hear it).  The definition above with two sentences changed:
 *  1. The signals are those of ss_add_pcm_channels (channel c alone, no mixdown).  The spec head runs on the plan's windows of every
 *     channel -- the windows of all channels fill the passes of ss_set_chunk_windows together -- and each channel has its own averaged
 *     maps: a float64 sum in ascending window order divided by the count, stored as float32, bit for bit what ss_separation_maps gives
 *     for that channel's file.
 *  3. STFT bin q of channel c gets channel c's gain.
 * Everything else is unchanged: the plan (ss_separation_plan), the default-step windows, the band gains, the triangles, the time
 * interpolation and its clamps, above_fmax, the fades, the encode, the transcode's bytes outside the intervals; all channels are
 * processed over the same merged intervals.  It acts as ss_reset + ss_add_pcm_channels of this file -- ss_reset_generation counts one
 * reset, afterwards files 0 .. channels - 1 are the channels; streams are untouched.  Arguments, output and refusals are
 * ss_separate_pcm's (SS_ERR_STATE on an audio-only context or while a run is in flight, SS_ERR_ARG for bad parameters, SS_ERR_RANGE
 * under SS_FLAG_F16X2 when any channel's passes leave the f16 range).  channels == 1 is ss_separate_pcm, byte for byte; so is a channel
 * without a partner (the last of an odd count) against ss_separate_pcm of its samples as a mono file, and a recording whose channels
 * hold the same samples against ss_separate_pcm of that recording. */
int ss_separate_pcm_channels(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames,
                             const ss_region* regions, int64_t n_regions, const ss_separation_params* params, int16_t* out);

/* ---- source output: silenced audio in the recording's own sample encoding -------------------------------------------------
 * ss_silence_pcm, ss_separate_pcm and ss_separate_pcm_channels end in the reference's sf.write(path, data, sr): 16-bit PCM whatever the
 * recording was (a 16-bit source comes back moved by one LSB at half of its codes, a 24-bit or float one loses its depth, floats beyond
 * +-1 wrap).  The *_source calls keep the encoding: outside the erased intervals the output is the input's bytes, inside them it is the
 * same audio in the same encoding.  fmt is the recording's enum ss_pcm_format, fb = channels x bytes per sample the frame size; the
 * merged frame ranges of a region table are ss_silence_pcm's (Python round, clamped to the file, merged).  `out` takes frames x fb
 * bytes; SS_ERR_CAPACITY when cap_bytes is smaller.
 *   Zeroing (ss_silence_pcm_source).  A byte whose frame lies in no range is the input byte -- nothing is decoded, so NaN payloads, -0.0,
 *   out-of-range floats and denormals pass through --; a byte whose frame lies in a range is the encoding's zero: 0x80 for SS_PCM_U8, 0x00
 *   for the other eleven.  Any context will do (audio-only included).
 *   Encode of a float32 y.  An integer format of b bits has S = 2^(b-1): q = rint(y x S), the product in float32 (exact: a power of two),
 *   rounded to nearest even, SATURATED to [-S, S - 1]; a NaN gives 0.  U8 stores q + 128, S8 q.  F32 stores y's bits, F64 (double)y.  The
 *   big-endian formats 7-12 store the same value with its bytes reversed.  The scale is the decode's own 2^(b-1), not 2^(b-1) - 1, so an
 *   8-, 16- or 24-bit sample that goes through decode and encode unchanged comes back as itself; saturation in place of the 16-bit
 *   path's wrap is deliberate (the 16-bit path keeps its wrap).
 *   Separation (ss_separate_pcm_source, ss_separate_pcm_channels_source).  Steps 1-3 of the separation silencer and step 4's
 *   y = x + w (p - x) unchanged; inside a merged interval every sample is the encode of y, outside the bytes are the input's.  State,
 *   refusals and reset counting are ss_separate_pcm's and ss_separate_pcm_channels'. */
int ss_silence_pcm_source(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames,
                          const ss_region* regions, int64_t n_regions, void* out, int64_t cap_bytes);
int ss_separate_pcm_source(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames, const ss_region* regions,
                           int64_t n_regions, const ss_separation_params* params, void* out, int64_t cap_bytes);
int ss_separate_pcm_channels_source(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames,
                                    const ss_region* regions, int64_t n_regions, const ss_separation_params* params, void* out,
                                    int64_t cap_bytes);
/* The 44-byte RIFF/WAVE header in front of such output for the little-endian encodings 1-6: format tag 1 (PCM) or 3 (IEEE float); for
 * SS_PCM_S16 it is ss_wav_header_pcm16's.  SS_ERR_ARG for the encodings 7-12 (AIFF's) and for a data chunk of 4 GiB or more.  Host only. */
int ss_wav_header(int format, int sample_rate, int channels, int64_t frames, void* out44);

/* Streams.  ss_stream_open_source opens a stream with output (ss_stream_open_output; each_channel != 0: ss_stream_open_channels' lanes)
 * whose output stays in the stream's own encoding; erase == NULL: pad_s = min_len_s = 0.  ss_stream_output_bytes reads it:
 * frames [*first_frame, *first_frame + *n_frames) as *n_frames x fb bytes (out == NULL asks for the two counts; SS_ERR_CAPACITY when
 * cap_bytes is smaller).  Equality: the concatenation of everything it returned equals, byte for byte,
 *     ss_silence_pcm_source(the whole recording, E(R)),    R = the regions the same stream returned;
 * the limit rule (ss_stream_output_limit), the bound D, the carried state and the refused-step behaviour are the streaming silencer's.
 * ss_stream_output on such a stream, and ss_stream_output_bytes on any other, answer SS_ERR_STATE.  A step that holds no such stream
 * makes exactly the launches it made before; 16-bit and source-output streams may share a step.
 * Images: such a stream exports "SSSTRM06" (those eight bytes, then the "SSSTRM03" / "SSSTRM04" image of the same stream with 16-bit
 * output, whole); every other stream writes the image it wrote before, and ss_stream_import reads all six.  Band streams have no
 * source output. */
int ss_stream_open_source(ss_ctx* ctx, int format, int sample_rate, int channels, double threshold, double break_s,
                          const ss_stream_erase* erase, int each_channel, int* stream_id);
int ss_stream_output_bytes(ss_ctx* ctx, int stream_id, void* out, int64_t cap_bytes, int64_t* first_frame, int64_t* n_frames);

/* ---- region bands: the frequency extent of the speech inside each region, from the spec head -----------------------------
 * The reference's Raven table gives every detection the box 0 .. 8000 Hz (review_exporter.py, low_freq / high_freq).  The spec head's
 * speech map says where in the 128 mel bands the voice sits; this section reduces it, on the device, to the measures Raven users work
 * with: the 5 % / 95 % energy frequencies and the peak frequency.  For a file already added (each-channel form: the files
 * first_file .. first_file + n_channels - 1 of ss_add_pcm_channels*) and n caller-given regions (ss_region: seconds, the "-3" applied):
 *  1. Bins of a region.  Bin j is centred at t_j = (j + 0.5) 3 / 256 - 3 s and belongs to [start, end) when start <= t_j < end: the
 *     first bin and the exclusive end are ceil((x + 3.0) * 256.0 / 3.0 - 0.5) for x = start and x = end, evaluated in double from left
 *     to right (no two of its operations can contract into an FMA), clamped to the covered bins [0, n_bins) of the file (the whole-file
 *     average's bins, ss_separation_plan_info.n_bins).  A region of the detector's own "%.4f" table keeps its bins under that
 *     rounding: half a bin is 5.9 ms.  Regions may overlap, repeat, come in any order or be empty; a region without a bin gets "no
 *     estimate" (step 4), which is no error.  SS_ERR_ARG for a region that is not finite or has end < start.
 *  2. Maps.  Step 1 of the separation silencer, unchanged: default-step (0.6 s) windows whatever ss_set_window_step says, the spec
 *     head on exactly the windows that cover a needed bin, a float64 sum in ascending window order divided by the count, stored as
 *     float32 -- bit for bit what ss_separation_maps returns for those bins.
 *  3. Profile.  Per region, spec channel c and band m: E_c[m] = sum_j P(y_c[j][m]), P(y) = expm1(min(y * y * ln 10, 600)) in double
 *     (the power behind a feature value, as the silencer's step 2; the cap keeps any sum of fewer than 2^64 bins finite); a NaN y
 *     adds 0, an infinite one the cap.  The order of the sum is fixed: the bins of a region are grouped into tiles by their absolute
 *     number j >> 6, a tile's sum is a sequential ascending float64 sum, and a region's tile sums are added in ascending tile order.
 *     So the work may be cut at tile boundaries, into as many pieces as memory asks for, without changing a bit.
 *  4. Bounds, on the speech channel (params->speech_channel, default 1 as in ss_separation_params): C[m] = C[m - 1] + E[m], sequential
 *     and ascending, T = C[127]; band_low is the smallest m with C[m] >= q_low T, band_high the smallest m with C[m] >= q_high T,
 *     band_peak the argmax of E (the lowest index on ties).  In Hz, with f[0 .. 129] the front-end's 130 HTK mel points
 *     (ss_band_edges: the float32 recipe of its filterbank, as doubles): low_hz = f[band_low] (the triangle's lower edge),
 *     high_hz = f[band_high + 2] (its upper edge), peak_hz = f[band_peak + 1].  speech_share = T_speech / (T_speech + T_env), T_env
 *     the same sequential sum over the other channel; n_bins = the bins used.  With T == 0 or n_bins == 0 the three band indices are
 *     -1 and the three frequencies and the share NaN: "no estimate", consumers fall back to their constants.
 *     Parameters: 0 < q_low < q_high <= 1 (defaults 0.05 / 0.95), speech_channel 0 or 1; otherwise SS_ERR_ARG. */
typedef struct ss_band_params {
    double q_low, q_high;              /* defaults 0.05, 0.95 */
    int32_t speech_channel, reserved;  /* default 1; reserved: 0 */
} ss_band_params;                      /* NULL params: the defaults */

typedef struct ss_region_band {
    double low_hz, high_hz, peak_hz, speech_share;
    int32_t band_low, band_high, band_peak, n_bins;
} ss_region_band;                      /* 48 bytes */

/* Host only: the 130 mel points f of step 4. */
int ss_band_edges(double* hz130);
/* Host only: rule 1 for one region of a file with covered_bins covered bins: *first = its first bin, *count = its bins (0: empty; then
 * *first is the clamped position of the start).  SS_ERR_ARG for a region that is not finite or has end < start, covered_bins < 0 or a
 * NULL pointer. */
int ss_region_bins(double start, double end, int64_t covered_bins, int64_t* first, int64_t* count);
/* Steps 1 - 4: out[n][n_channels], profile (NULL, or [n][n_channels][2][128]: E of both spec channels in the head's order).
 * n_channels == 1: the file first_file.  State rules and refusals are ss_separation_maps': the files are already added and stay,
 * nothing is reset; SS_ERR_STATE on an audio-only context or while a run is in flight; SS_ERR_RANGE under SS_FLAG_F16X2 when the spec
 * head's passes leave the f16 range (run the file in an fp32 context), with `out` not to be used.  n == 0 is SS_OK.  The last run's
 * region tables (ss_get_regions*) stay readable; what reads the run's device buffers (ss_get_window_logits, ss_get_avg,
 * ss_get_region_peaks) answers SS_ERR_STATE afterwards, as after ss_separation_maps or ss_infer_windows -- the passes reuse those
 * buffers --, whenever a region had a bin: read them first.  Long tables are worked through
 * in pieces of a fixed number of bins, cut at tile boundaries (step 3): the result does not depend on the cuts. */
int ss_region_bands(ss_ctx* ctx, int first_file, int n_channels, const ss_region* regions, int64_t n, const ss_band_params* params,
                    ss_region_band* out, double* profile);
/* Steps 1, 3 and 4 on maps the caller supplies (ss_separation_maps' layout per signal): maps[n_signals][2][n_bins][128] hold the bins
 * first_bin .. first_bin + n_bins - 1, and no other bin exists for this call (step 1 clamps to them).  out[n][n_signals], profile as
 * above.  Needs a device but no weights; SS_ERR_STATE while a run is in flight. */
int ss_region_bands_from_maps(ss_ctx* ctx, const float* maps, int n_signals, int64_t first_bin, int64_t n_bins, const ss_region* regions,
                              int64_t n, const ss_band_params* params, ss_region_band* out, double* profile);

/* ---- stream bands: each final region's frequency extent as a stream returns it ------------------------------------------------
 * A stream opened with ss_stream_open_bands returns, with every region ss_stream_regions returns, that region's ss_region_band (and,
 * with want_profile, its profile), in the same step as the region: no new latency bound.
 * Equality.  Let R be the concatenation of the regions the stream returned, Bs and Ps of the bands and profiles.  Bs and Ps equal, as
 * bytes (NaNs by bit pattern), `out` and `profile` of ss_region_bands(ctx', first_file, C, R, n, params, out, profile) after ss_add_pcm
 * + ss_run of the whole recording on a context ctx' of the same precision; an each-channel stream of C channels is compared with
 * ss_add_pcm_channels and out[n][C], every channel under the merged table.  This holds for any split into pieces and any cadence of
 * steps, whichever other streams (of any kind, with or without bands) shared the steps, and across ss_stream_export / ss_stream_import
 * between contexts of the same precision.  Steps 1 - 4 of "region bands" apply unchanged: rule 1 on the ss_region values the stream
 * returns; the maps as float64 sums over a bin's covering default-step windows in ascending window order, divided by the count, stored
 * as float32 (0 for a bin no window covers, which exists only behind the last window of a closed stream); P(y), the cap at 600, NaN
 * adds 0, tiles by j >> 6; the sequential C, the quantiles, the first argmax, the Hz edges and "no estimate" as they stand.
 * Everything else the stream returns (regions, averages, peaks, output) is bit for bit what the same stream returns with bands off,
 * and streams without bands run in passes of their own, which make exactly the launches of a context that never saw a band stream.
 * State (counted by ss_stream_info.state_bytes), bounded and independent of the stream's and of any region's length.  Per lane (one
 * lane; one per channel of an each-channel stream): five vectors of 256 doubles (10 KB) -- the sum of the candidate region's completed
 * tiles, the running sum of its current tile, a snapshot of both taken before the candidate's current last bin (its exclusive end under
 * rule 1), and the profile of a region that is final but not returned yet --, and the float64 map sums of the bins that a window
 * already covers but that are not final: 2 KB per bin for at most the 256 bins of a window plus the bins of one step (51.2) and of the
 * resampler's look-ahead, about 0.6 MB.  break_s adds nothing: a gap is walked through, not held.
 * Refusals.  SS_ERR_STATE: a context whose window step is not the default 0.6 s (the maps are defined on default-step windows), an
 * audio-only context, ss_stream_bands on a stream without bands, `profile` on a stream opened without want_profile.  SS_ERR_ARG:
 * params as in ss_region_bands.  Under SS_FLAG_F16X2 a step whose passes -- the spec head's among them -- set the range flag returns
 * SS_ERR_RANGE and commits nothing, band state included.
 * Images.  A stream with bands exports "SSSTRM05" (the content of the older images plus the band parameters, the accumulators and the
 * carried map sums; a finished stream carries none, its image holds zeros there); every other stream writes the image it always wrote;
 * ss_stream_import reads all five.  An "SSSTRM05" image that
 * does not hold together -- a wrong length, a bad lane count or parameters, a step other than the default -- is SS_ERR_ARG. */
/* The one open call that expresses every combination (erase / with_output as ss_stream_open_channels; each_channel != 0: one lane per
 * channel; params NULL: the defaults).  The three older open calls keep bands off. */
int ss_stream_open_bands(ss_ctx* ctx, int format, int sample_rate, int channels, double threshold, double break_s,
                         const ss_stream_erase* erase, int with_output, int each_channel, const ss_band_params* params, int want_profile,
                         int* stream_id);
/* The last step's records out[n][lanes] (and profile, NULL or [n][lanes][2][128]) for the n regions ss_stream_regions returns; both
 * NULL: *n_out alone.  SS_ERR_CAPACITY when cap_regions < n. */
int ss_stream_bands(ss_ctx* ctx, int stream_id, ss_region_band* out, double* profile, int64_t cap_regions, int64_t* n_out);

/* ---- separation streams: the rule ----------------------------------------------------------------------------------------------
 * The missing cell beside ss_silence_pcm, ss_stream_open_output and ss_separate_pcm is a stream with output whose output is separated
 * instead of zeroed: everything it returns, concatenated, is to equal, byte for byte,
 *     ss_separate_pcm(the whole recording, ss_erase_table(R, erase), params),   R = the regions the same stream returned.
 * This header holds the host side of it -- which frames a step of such a stream may return as final, and how far they lag -- so that the
 * rule stands and is tested without a GPU (tests/test_stream_separate_host.py).  The stream itself (an open call, the kernels, the
 * image) is not built: see DESIGN.md section 20.
 *
 * Which frames a step may return (ss_stream_separate_limit).  With F = round(fade_s x sample_rate), N and hop = N / 4 the STFT's, b the
 * final bins, H the frames decoded and Lz = ss_stream_output_limit(...) clamped to [0, H], a frame n may be returned before the close
 * when
 *   1. n < Lz - F.  Its blend weight w(min(n - a, e - 1 - n)) is decided.  Membership and the interval's start a are decided below Lz
 *      (the zeroing rule).  The end e is not: a pending region that passes the filter grows (e >= Lz); an interval that ends at or
 *      behind Lz can be joined by a later padded region that touches it (break_s < 2 pad_s), which removes its fade-out; the end of the
 *      recording clamps e to a value >= H >= Lz.  In every case e >= Lz now and later, so e - 1 - n >= F and the weight is
 *      w(min(n - a, F)).  An interval that ends below Lz is final: no later region starts below Lz.
 *   2. n + N <= H.  The STFT frames floor(n / hop) - 1 .. + 2 over n read samples below n + N; the zeros behind the recording are
 *      known only at the close.
 *   3. STFT frame floor(n / hop) + 2 reads, unclamped, the bins j0, j0 + 1 <= b - 1: its gains (and those of the three frames before
 *      it) are final, and the clamp to the last covered bin -- known only at the close -- does not act, since every final bin of an
 *      open stream is a covered bin of the whole file.
 * A step may return [frames_out, min(max(limit, frames_out), H)), limit the smallest of the three; the close returns the rest.
 * Latency.  Such a frame at audio time t is returned by the first step after the stream holds audio past t + D_sep,
 *     D_sep = D + fade_s + (N + 1) / sample_rate            (ss_stream_separate_latency; D of the streaming silencer):
 * condition 1 costs F frames behind Lz >= H - D, condition 2 N frames, condition 3 less than B + N / sample_rate <= D + N / sample_rate
 * (the frame two hops ahead must lie half a bin below the first non-final bin). */
/* Host only: the limit frame of the rule above (the smallest of its three conditions), before the clamp to [frames_out, frames
 * decoded]; it may be negative.  pending / pending_start / pending_end as ss_stream_output_limit; params as ss_separation_plan
 * validates them (NULL: the defaults).  INT64_MIN on a bad argument. */
int64_t ss_stream_separate_limit(int sample_rate, int64_t frames_decoded, int64_t bins_final, int pending, double pending_start,
                                 double pending_end, const ss_stream_erase* erase, const ss_separation_params* params);
/* Host only: D_sep in seconds; NaN on a bad argument. */
double ss_stream_separate_latency(int sample_rate, double break_s, const ss_stream_erase* erase, const ss_separation_params* params);

/* ---- band silencer: erase only each region's own frequency band ------------------------------------------------------------
 * The third silencing method, between the other two: ss_silence_pcm zeroes the whole spectrum of a reviewed interval, ss_separate_pcm
 * needs the network.  This one works from a table of boxes alone -- the region bands' side file, or boxes adjusted by hand --: inside
 * each box's time range the box's own frequency band is removed and the rest of the spectrum stays.  No model pass; any context will
 * do.  Definition (float64 restatement: tests/box_ref.py), step by step:
 *  1. Time ranges.  Box i has the frame range [a_i, b_i): ss_silence_pcm's rounding (Python round of start x sample_rate and end x
 *     sample_rate), clamped to the file; a box whose range is empty drops out.  The merged intervals are the merge of all [a_i, b_i),
 *     on whichever channel they act, as ss_silence_pcm merges (overlapping and touching ranges join).
 *  2. STFT.  Step 3 of the separation silencer, unchanged: N = the separation silencer's FFT size of the rate, hop N / 4, periodic Hann
 *     for analysis and synthesis, the overlap-add divided by 1.5, frame k centred on sample k hop, zeros outside the file.  Only the
 *     frames whose support meets a merged interval run.
 *  3. Gains.  Frame k is active for box i when its support [k hop - N/2, k hop + N/2) meets [a_i, b_i): every sample inside a box has
 *     all four of its frames active for that box.  With lo_b = low_hz N / sample_rate, hi_b = high_hz N / sample_rate (a NaN low_hz
 *     counts as 0, a NaN high_hz as +infinity: "no estimate" erases the whole band), e_b = edge_hz N / sample_rate,
 *     q_lo = ceil(lo_b) and q_hi = min(floor(hi_b), N/2) -- both decided on the host in double --, the profile of box i over the STFT
 *     bins q = 0 .. N/2 is
 *         v_i(q) = 1                                   for q_lo <= q <= q_hi,
 *                  (1 + cos(pi d / e_b)) / 2           for q < q_lo with d = lo_b - q < e_b, and for q > q_hi with d = q - hi_b < e_b,
 *                  0                                   otherwise (e_b = 0: the hard edge),
 *     its gain g_i(q) = 1 - (1 - min_gain) v_i(q), and G_c(k, q) = the minimum of g_i(q) over the boxes active at k that act on channel
 *     c (channel -1: on every channel), 1 when there is none.  The gain is real and even in q.
 *  4. Blend and encode.  Step 4 of the separation silencer: y = x + w (p - x) with the raised-cosine ramp over round(fade_s x
 *     sample_rate) samples at either end of a MERGED interval; lrintf(y x 32767) for the 16-bit call, the source output's encode for
 *     the _source call.  Outside the merged intervals the output is ss_silence_pcm's transcode / the input's bytes.
 * With a full-band box (low 0 or NaN, high >= sample_rate / 2 or NaN) on every channel, min_gain 0 and fade_s 0 the output is
 * ss_silence_pcm's (ss_silence_pcm_source's), byte for byte.
 * State: ss_silence_pcm's.  Any context (audio-only included); the job's files, results and streams are untouched; SS_ERR_STATE while a
 * run is in flight.  SS_ERR_ARG: a start or end that is not finite, end < start, low_hz > high_hz (after the NaN rule), a negative
 * high_hz, a channel outside -1 .. channels - 1, reserved != 0, fade_s or edge_hz negative or not finite, min_gain outside [0, 1].
 * n_boxes == 0, or boxes that are all empty: the plain transcode / the input's bytes. */
typedef struct ss_box {
    double start, end;          /* seconds, as ss_region (the reference's "-3" applied) */
    double low_hz, high_hz;     /* NaN low_hz: 0; NaN high_hz: +infinity */
    int32_t channel;            /* -1: every channel; 0 .. channels - 1: that channel alone */
    int32_t reserved;           /* 0 */
} ss_box;                       /* 40 bytes */

typedef struct ss_box_params {
    double fade_s;              /* >= 0, default 0.01 */
    double min_gain;            /* in [0, 1], default 0 */
    double edge_hz;             /* >= 0, default 100: the raised-cosine roll-off outside [low_hz, high_hz] */
} ss_box_params;                /* NULL params: the defaults */

typedef struct ss_box_range {   /* one merged interval and the STFT frames whose support meets it */
    int64_t frame_begin, frame_end;    /* [begin, end) */
    int64_t stft_first, stft_last;     /* inclusive; stft_first may be negative */
} ss_box_range;

typedef struct ss_box_plan_info {
    int32_t n_fft, hop;
    int64_t n_frames;                  /* STFT frames whose support meets a merged interval, each counted once */
    int64_t n_ranges;                  /* out: merged intervals */
    int64_t cap_ranges;                /* in: room in `ranges` (SS_ERR_CAPACITY when smaller; n_ranges is set either way) */
    ss_box_range* ranges;              /* in: caller's array (NULL when cap_ranges == 0) */
} ss_box_plan_info;

/* Host only: the plan of ss_box_silence_pcm for a file of `frames` frames at sample_rate (the limits of ss_add_pcm).  The channel field
 * of a box is checked against -1 .. 255 here (the file's channel count is not an argument); everything else as the calls below. */
int ss_box_plan(int sample_rate, int64_t frames, const ss_box* boxes, int64_t n_boxes, const ss_box_params* params, ss_box_plan_info* out);
/* The band silencer (above): interleaved PCM in (any enum ss_pcm_format, rate and channel count ss_add_pcm takes), interleaved 16-bit
 * PCM out (frames x channels int16, as ss_silence_pcm). */
int ss_box_silence_pcm(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames, const ss_box* boxes,
                       int64_t n_boxes, const ss_box_params* params, int16_t* out);
/* The same in the recording's own encoding (source output: `out` takes frames x channels x bytes per sample bytes, SS_ERR_CAPACITY
 * when cap_bytes is smaller; every byte outside the merged intervals is the input's). */
int ss_box_silence_pcm_source(ss_ctx* ctx, const void* pcm, int format, int sample_rate, int channels, int64_t frames, const ss_box* boxes,
                              int64_t n_boxes, const ss_box_params* params, void* out, int64_t cap_bytes);

/* ---- measurement ---------------------------------------------------------------------------- */
/* Enqueue-only variant of ss_run used by bench.py: same work, no host readback until ss_sync. */
int ss_sync(ss_ctx* ctx);
int ss_reset_kernel_stats(ss_ctx* ctx);
int ss_get_kernel_stats(ss_ctx* ctx, ss_kernel_stat* out, int cap, int* n_out);
/* elapsed device time of the last ss_run between its first and last kernel (HIP events on the
 * context's stream), milliseconds */
double ss_last_run_device_ms(ss_ctx* ctx);
/* bytes of device memory the context's activation workspace holds (0 after a failed growth) */
int64_t ss_workspace_bytes(ss_ctx* ctx);

#ifdef SS_DEVBUILD
/* ---- development build only (libsoftspoken_hip_dev.so, -DSS_DEVBUILD): not exported by the product library ----------- */
/* Fault injection for the tests: the nth (0-based) allocation of the next activation-workspace growth fails with an out-of-memory
 * error; nth < 0 switches it off.  The context must come out of such a failure without a workspace (and allocate one afresh on
 * the next call), never with dangling tensors. */
int ss_debug_fail_workspace_alloc(ss_ctx* ctx, int nth);
/* ss_separate_pcm (and ss_box_silence_pcm) holds at most `frames` resynthesised STFT frames at once (never fewer than 16) in place of the number that fits its
 * 256 MB frame buffer, so that a short recording meets the cuts of a long one: a chunk ends when the next piece would pass the number,
 * an interval is cut into pieces of (frames - 8) hops.  frames <= 0: the product's number again.  The bytes written must not depend on it. */
int ss_debug_set_separation_budget(ss_ctx* ctx, int64_t frames);
/* ss_region_bands covers at most `bins` bins (never fewer than 64) with one round of network passes, in place of the product's fixed
 * number, so that a short recording meets the cuts of an hour of speech.  Pieces are cut at tile boundaries (absolute multiples of 64
 * bins) only; a region may span pieces, its tile sums wait on the device until its last piece is done.  bins <= 0: the product's
 * number again.  The bytes written must not depend on it. */
int ss_debug_set_bands_budget(ss_ctx* ctx, int64_t bins);
/* Activation tensors of the context's last network pass, for per-launch tests.  name: a tensor of the activation workspace ("h1" ... "s9"),
 * "feat" (the pass's features) or "flat_part" (conv_flatten's row-group partial sums, fp32 [n][groups][4][256] read as H = groups,
 * W = 4, C = 256; exponents: the common power of two they carry).  Copies windows [first_window, first_window + n_windows) of one plane as [n][H][W][C], whatever the stored
 * byte order (the f16x2 tensors wider than 32 channels are stored [n][C / 32][H][W][32] and gathered on readback): fp32,
 * bf16, or under SS_FLAG_F16X2 the high (plane 0) or low (plane 1) f16 halves.  shape (if not NULL) receives H, W, C and the bytes of
 * one element; exponents (if not NULL, C entries) the power-of-two channel exponents of the tensor (the stored value of channel c is
 * 2^e[c] x its value; all zero outside SS_FLAG_F16X2).  out == NULL: shape and exponents only, for any tensor of the model (no pass
 * needed).  With out given (n_windows may be 0: the checks alone): SS_ERR_STATE without a workspace, while a run is in flight, after a
 * pass on the second lane, and for a tensor the last pass did not write; then SS_ERR_ARG for an "r*" tensor (stored in MFMA fragment
 * order: the pass wrote it, i.e. ran that block as A + r / B), an unknown name, a plane the mode does not have, windows outside the
 * last pass or a short buffer. */
int ss_debug_activation(ss_ctx* ctx, const char* name, int plane, int64_t first_window, int64_t n_windows, void* out, int64_t out_bytes,
                        int32_t* shape, int32_t* exponents);
#endif

#ifdef __cplusplus
}
#endif
#endif /* SOFTSPOKEN_H */
