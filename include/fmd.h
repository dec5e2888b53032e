/*
 * fmd.h -- C ABI of the MI355X-native FM broadcast decoder (libfmd_hip.so).
 *
 * Drop-in boundary for ONE path of AlwinEsch/pvr.rtl.radiofm: cFmDecoder::ProcessStream()
 * and the upward RDS callbacks.  The reference has no C ABI for this path (cFmDecoder is a
 * hidden C++ class, src/FmDecode.h:91); the entry points below are what a binding of that
 * class would need, one per reference member, plus batched variants (many independent
 * channels per call) which are what the GPU is for.  include/fm_decoder.hpp puts the
 * reference's exact class surface on top of this ABI.
 *
 * All citations are relative to /root/reference/src/.  Plain pointers and sizes only; no
 * torch / HIP types (streams are passed as void* = hipStream_t).  Every function returns
 * FMD_OK or a negative error; fmd_last_error() gives the text.  There is no CPU fallback:
 * if no HIP device is usable the create calls fail.
 */
#ifndef FMD_H
#define FMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMD_OK 0
#define FMD_ERR_ARG (-1)     /* invalid argument / unsupported configuration */
#define FMD_ERR_DEVICE (-2)  /* HIP runtime error or no usable device */
#define FMD_ERR_SIZE (-3)    /* samples outside [fmd_batch_min_samples(), FMD_MAX_BLOCK] */
#define FMD_ERR_STATE (-4)
/* Not an error (positive): RDS groups were lost since the last report -- a call's group queue or the
 * record buffer of fmd_batch_export_rds_device was full.  Audio and channel state are intact and the
 * batch stays usable.  Returned once by fmd_batch_wait[_lagged] / fmd_batch_export_rds_device (or
 * queried with fmd_batch_take_rds_lost), then cleared.  The reference has no such condition: its
 * group decoder runs inside ProcessStream (RDSProcess.cpp:312,355), nothing is ever queued. */
#define FMD_WARN_RDS_LOST 1

/* cRtlSdrSource::default_block_length (RTL_SDR_Source.h:25): the reference's internal buffers
 * are hard-sized to it (FmDecode.cpp:277-282), so samples <= 65536 is its precondition too. */
#define FMD_MAX_BLOCK 65536u
/* Calls of at least this size are taken by every geometry.  The exact lower bound of a batch is
 * fmd_batch_min_samples() and is far smaller (88 samples at 2.4 MS/s / downsample 11): short blocks
 * are decoded the way the reference decodes them -- a half-band stage with fewer than L inputs
 * passes them on unfiltered (DownConvert.cpp:519-520), with fewer than 2 (L - 1) it refills its delay
 * line from its own outputs (:546-547, the in-place array), a block shorter than a filter keeps part
 * of the old history (:137-145, :236-253).  Refused (FMD_ERR_SIZE) are only blocks so short that some
 * stage would get no sample at all -- the reference's level meters divide by zero there
 * (FmDecode.cpp:522-539) -- or fewer than the 20 inputs its unrolled 11-tap stage reads
 * unconditionally (:596-661). */
#define FMD_MIN_BLOCK 8192u
/* A further limit inherited from the reference: samples / downsample (the baseband length of a
 * call) must stay below 32768 - 51, the size of its half-band delay lines (DownConvert.cpp:267,
 * :500; it overruns them silently).  Only matters for downsample < 3. */

/* IQ input formats: the `format` argument of the _fmt entry points.  I and Q interleaved, host byte order.
 *   FMD_IQ_F32  float I, Q      as is                                         8 bytes per IQ sample
 *   FMD_IQ_U8   uint8_t I, Q    float(b / (255.0 / 2.0) - 1.0) (RTL-SDR, see fmd_process_stream_u8)   2
 *   FMD_IQ_S8   int8_t I, Q     (float)v * 2^-7   (HackRF, .cs8 files)                               2
 *   FMD_IQ_S16  int16_t I, Q    (float)v * 2^-15  (Airspy, SDRplay, USRP sc16, .cs16 files)          4
 * The conversion happens inside the IF kernel (and the scan's first pass).  The two signed conversions are exact
 * in float, so a call with S8 / S16 input gives the same bits in every output as the float call on the block
 * converted on the host; -128 and -32768 are exactly -1.0f.  The scale is fixed: a receiver that leaves 12 or 14
 * bits right-aligned in an int16 decodes correctly and only reads 24 / 12 dB low on interface_level (a
 * caller-chosen scale or per-batch gain is not offered).
 * Alignment: IQ pointers and channel / capture strides are multiples of two IQ samples -- 16 bytes of F32, 4
 * bytes of U8 and S8, 8 bytes of S16.  Strides are counted in IQ samples for every format.
 * The format is a property of the call, not of the batch, the decoder, the receiver or the scan: all state behind
 * the tuner is float, so consecutive calls may use different formats.
 * A format outside 0..3 is refused with FMD_ERR_ARG before anything else is looked at.  The functions without
 * _fmt (float input) and with _u8 remain and are calls of the _fmt ones with FMD_IQ_F32 / FMD_IQ_U8. */
#define FMD_IQ_F32 0
#define FMD_IQ_U8 1
#define FMD_IQ_S8 2
#define FMD_IQ_S16 3
/* Real-sampled input, for a real band splitter only (fmd_split_create_real, below): one element per sample,
 * 16 | the FMD_IQ_* of the same element type, converted like its I part (exact for the integers):
 *   FMD_REAL_F32  float    as is              4 bytes per sample
 *   FMD_REAL_S8   int8_t   (float)v * 2^-7    1
 *   FMD_REAL_S16  int16_t  (float)v * 2^-15   2    (Airspy raw mode, direct-sampling ADC boards)
 * 17 is not a format (no unsigned real samples).  Every entry point but fmd_split_process_* of a real splitter
 * refuses these values like any other value outside 0..3. */
#define FMD_REAL_F32 16
#define FMD_REAL_S8 18
#define FMD_REAL_S16 19

/* Audio output formats: the `pcm_format` argument of the _pcm entry points.  L and R interleaved, host byte order.
 *   FMD_PCM_F32  float L, R     what cFmDecoder::ProcessStream hands its caller; the default everywhere   4 bytes
 *   FMD_PCM_S16  int16_t L, R   saturate_int16(round_half_even(x * 32768.0f)), NaN gives 0                2
 * where x is the float sample the FMD_PCM_F32 call writes: x * 2^15 is exact in float (short of overflow, which
 * saturates), so every sample has one right value -- 1.0 gives 32767, -1.0 gives -32768, 0.5 / 32768 gives 0,
 * 1.5 / 32768 and 2.5 / 32768 give 2.  No dither and no gain argument: the scale is fixed like the input's.  The
 * conversion happens in the registers of the audio tail kernel (fmd_f32_to_s16, csrc/fmd_math.h); half the bytes
 * leave the device.  The same number of samples per channel as the float call; strides and sample counts are in
 * elements of the format.  Everything else a call produces -- channel state, status record, the audio meter
 * (its sums are taken over the float samples), RDS groups -- is the bits of the same call with FMD_PCM_F32, and
 * the format is a property of the call: calls of either format may follow each other freely.
 * Stereo programme material overshoots full scale now and then (the stereo lock's transient; over-deviated
 * stations all the time): fmd_batch_read_pcm_clipped counts the samples that saturated.
 * A format outside 0..1 is refused with FMD_ERR_ARG before anything else is looked at.  The functions without
 * _pcm remain and are calls of the _pcm ones with FMD_PCM_F32. */
#define FMD_PCM_F32 0
#define FMD_PCM_S16 1

/* The demodulated multiplex (MPX) beside the audio: the `mpx_format` argument of the _mpx entry points.  The
 * multiplex is the FM PLL's output at the baseband rate (m_BufferBaseband, FmDecode.cpp:433) -- what an external
 * RDS / RDS2 / DARC / SCA decoder, a modulation analyser or a stereo decoder of the caller's own consumes, and the one
 * signal worth archiving when a station is to be decoded again later.  Mono, one row per channel, host byte order:
 *   FMD_MPX_F32  float     the sample as is                                                       4 bytes
 *   FMD_MPX_S16  int16_t   saturate_int16(round_half_even(x * 8192.0f)), NaN gives 0              2
 * Content: sample t of a call's row is the float FMD_TAP_BASEBAND returns at t, bit for bit; a call delivers
 * M = *out_mpx_samples of them, the call's baseband length, the same for every channel, known when the call returns
 * and at most fmd_batch_max_mpx_samples(b, samples).
 * Scale: a carrier deviation of f Hz reads x = f / 30 000 (FmDecode.cpp:254, :409-412): +-75 kHz is +-2.5.  The DC
 * term (the tuning offset) is already removed there; nothing else is applied -- no de-emphasis, no filter, no
 * resampling.  FMD_MPX_S16: full scale is +-4.0 = +-120 kHz, +-75 kHz is +-20 480; x * 2^13 is exact in float short
 * of overflow, which saturates, so every sample has one right value.  There is no clip counter: a saturated sample
 * reads 32767 or -32768, and whoever receives the row can count those.
 * Rate: fmd_batch_mpx_rate(b) = sample_rate_if / downsample samples per second (218 181.8 at 2.4 MS/s and 11).
 * The format is a property of the call: calls without multiplex, with FMD_MPX_F32 and with FMD_MPX_S16 may follow
 * each other freely, and a call that asks for the multiplex leaves channel state, audio, status record, audio meter
 * and RDS groups with the bits of the same call without it.  A channel that was reset, retuned or moved to another
 * capture in front of the call delivers the multiplex of the decoder it now is.
 * A format outside 0..1 is refused with FMD_ERR_ARG before anything else is looked at. */
#define FMD_MPX_F32 0
#define FMD_MPX_S16 1

/* The mono feed beside the audio: the `feed_format` argument of the _feed entry points.
 * Speech-to-text, fingerprinting and loudness logging take mono at 16 or 24 kHz; the feed is every channel's mono mix,
 * low-passed and decimated by D = 2 or 3 (fmd_batch_set_feed) on the device, one row per channel, host byte order:
 *   FMD_FEED_F32  float     the filter's sum y as is                                              4 bytes
 *   FMD_FEED_S16  int16_t   fmd_f32_to_s16(y): FMD_PCM_S16's rule, saturating, NaN gives 0        2
 * There is no clip counter: a saturated sample reads 32767 or -32768.
 * Definition, exact (no tolerance): for audio frame g of a channel x[g] = (L[g] + R[g]) * 0.5f in float, L and R the
 * floats the FMD_PCM_F32 call writes for that frame (a frame decoded as mono: the sample itself); g counts the frames
 * of the calls that asked for the feed since fmd_batch_set_feed, x[g] = 0 for g < 0.  Taps
 * h = make_kaiser_lp(1.0f, 60.0f, 0.425f * fo, 0.575f * fo, fs) with fs = (float)sample_rate_pcm, fo = fs / D in float
 * (fmd_design_lp_kaiser with these arguments; fmd_batch_get_feed_taps returns them): 49 taps for D = 2, 73 for D = 3,
 * stop band from 0.575 fo at -58 dB.  y[n] = sum over k = 0 .. T - 1 of h[k] * x[n D - k], accumulated in float from
 * acc = 0 with k ascending, acc = acc + h[k] * x[n D - k], multiply and add rounded separately: a numpy float32 loop
 * over k gives the same bits.  A call whose frames are g0 .. g0 + A - 1 delivers the outputs n with
 * g0 <= n D < g0 + A: ceil((g0 + A) / D) - ceil(g0 / D) samples, in order, the same number for every channel, known
 * when the call returns; it may be 0.
 * Rate: fmd_batch_feed_rate(b) = sample_rate_pcm / D (24 000 or 16 000 at 48 kHz).
 * The feed is the concatenation of the calls that asked for it: a call without it (d_feed == NULL) is a SPLICE in the
 * feed, not a gap of zeros -- its frames are never seen by the filter.  A call that asks for the feed leaves channel
 * state, audio, multiplex, status record, audio meter and RDS groups with the bits of the same call without it.
 * The feed belongs to the output like the audio meter and the clip counter: fmd_batch_reset, fmd_batch_reset_channels,
 * retunes, capture switches and imports leave its history and g alone (it goes on with whatever audio the slot now
 * produces); it is no part of a state blob and fmd_batch_load_state does not touch it.  Only fmd_batch_set_feed zeroes
 * it.  A format outside 0..1 is refused with FMD_ERR_ARG before anything else is looked at. */
#define FMD_FEED_F32 0
#define FMD_FEED_S16 1

/* The channel IQ beside the other outputs: the `ciq.format` of a call record (fmd_call).
 * It is every channel's complex baseband behind the tuner and the decimating IF filter (cFineTuner::Process +
 * cDownsampleFilter::Process, m_BufferIF) -- the samples the FM PLL demodulates: for a demodulator of the caller's
 * own, the envelope |z| the PLL discards, a station's own power, an archive at 1 / downsample of the capture's rate,
 * or the IF stage used as a bank of digital down-converters.  One row per channel, interleaved re, im, host byte order:
 *   FMD_CIQ_F32  float   re, im   the sample as is: the bits FMD_TAP_DEMOD returns                8 bytes a sample
 *   FMD_CIQ_S16  int16_t re, im   fmd_f32_to_mpx16 of each part: saturate_int16(round_half_even(x * 8192.0f)),
 *                                 NaN gives 0 -- literally the multiplex's conversion                 4
 * Length and rate: a call delivers M complex samples per row, M = the call's multiplex count, at most
 * fmd_batch_max_mpx_samples(b, samples), at fmd_batch_mpx_rate(b) samples per second; sample k of a row is the sample
 * whose PLL output is multiplex sample k.
 * Scale: the tuner's factor 2 is in the samples (full-scale float input gives |z| up to 2); FMD_CIQ_S16's full scale
 * is +-4.0.  There is no clip counter, as with the multiplex.
 * Units: strides and counts of this output are COMPLEX SAMPLES.
 * The format is a property of the call, and a call that asks for the rows leaves audio, multiplex, feed, status
 * records, meters, RDS groups, block records and channel state with the bits of the same call without them.  The rows
 * follow the slot: behind a reset, retune, capture switch, import or load they are those of the decoder the slot now
 * is, and under FMD_FIR_*_PARITY_WAIVED and every kernel form of the IF stage they are what that stage wrote.
 * A format outside 0..1 is refused with FMD_ERR_ARG before anything else is looked at.
 * fmd_debug_math has no entry of its own for the conversion: what = 9 is fmd_f32_to_mpx16, the one function both
 * writers call. */
#define FMD_CIQ_F32 0
#define FMD_CIQ_S16 1

/* The way back in: channel IQ rows as the INPUT of a call -- an archive made through `ciq`
 * decoded again, or the rows of a channeliser of the caller's own (a polyphase filter bank, an FPGA front end, a DDC in
 * the receiver).  Two more values of fmd_call.iq_format, taken by the three _call entry points only
 * (fmd_batch_process_device_call, fmd_batch_process_host_call, fmd_process_stream_call); every positional entry point,
 * the receiver, the scan and the splitter refuse them with FMD_ERR_ARG and a sentence, before anything else is touched:
 *   FMD_IN_CIQ_F32  float   re, im   as is: the bits FMD_CIQ_F32 and FMD_TAP_DEMOD deliver
 *   FMD_IN_CIQ_S16  int16_t re, im   (float)v * 2^-13 of each part (fmd_ciq16_to_f32): exact in float and the inverse
 *                                    scale of FMD_CIQ_S16 -- a call with S16 rows has the bits of the F32 call on the
 *                                    same rows converted by the host
 * Field meanings with these formats: `iq` is one row per channel, channel c reads row c, no capture map is consulted
 * and channels-per-capture does not apply; `iq_channel_stride` is in COMPLEX SAMPLES; `samples` is M, the baseband
 * length of the call (what fmd_batch_max_mpx_samples counts for an IQ call).
 * Device call: the pointer 16-byte aligned, the stride a multiple of 2 complex samples (F32) / 4 (S16), and >= M when
 * the batch has more than one channel -- the rules of the `ciq` output's rows.  Host call and single decoder: any
 * stride >= M and any alignment, through the input's staging buffer.
 * Which M: exactly those an IQ call producing that M would be accepted with, and the plan's sentences
 * (FMD_ERR_SIZE): too short for the RDS chain or for an audio frame, M + 51 > 32768, an odd M in front of CIC stages,
 * M above the batch's largest.  fmd_batch_baseband_limits has the numbers: *min = fmd_batch_min_samples / downsample,
 * *max = the decimator's outputs of the largest block, *multiple = 2 per CIC stage of the RDS decimator (else 1).
 * What such a call does: the IF stage does not run -- no tuner, no FIR, no level meter -- and its carried state (the
 * filter's history, the tuner's phase, the decimator's phase) is untouched: the next IQ call continues as if the
 * channel-IQ calls between had not happened.  Everything behind the IF stage takes the rows as that stage's output of
 * a call of baseband length M: audio in both PCM formats, multiplex, feed and `ciq` out (a copy of the input, F32
 * bits), status, audio meter and clip counters, RDS groups, block records and counters, UECP frames, selections and
 * debug taps (FMD_TAP_DEMOD returns the row).  interface_level, the one status field that reads raw IQ, keeps the
 * value the last IQ call left.  The kind belongs to the call like the formats: consecutive calls may differ, with calls
 * in flight.  Edits (resets, retunes, switches, imports, loads) are applied in front of the next call submitted as
 * ever; what they change in the IF stage is seen by the next IQ call.  State blobs are unchanged.  Non-finite rows
 * are decoded as the definition says, NaN for NaN, confined to their channel.  The input buffer is free when the
 * copying kernel (k_ciq_in, in the IF stage's place on its stream) has run: the rule of IQ input, also with
 * concurrency 2.  The tuner's factor 2 is in such rows (see FMD_CIQ_*): an external channeliser scales by 2. */
#define FMD_IN_CIQ_F32 32
#define FMD_IN_CIQ_S16 33

/* Constructor arguments of cFmDecoder (FmDecode.h:110-116).  table_size / if_filter_order are
 * the two internal constants BASELINE configs 3 and 5 override; 0 selects the reference
 * values 64 (FmDecode.cpp:249) and 8*downsample (FmDecode.cpp:262). */
#define FMD_FIR_SEQUENTIAL 0
#define FMD_FIR_SHUFFLE_PARITY_WAIVED 0x101
#define FMD_FIR_FMA_PARITY_WAIVED 0x102
typedef struct fmd_params
{
  double sample_rate_if;
  double tuning_offset;
  double sample_rate_pcm;
  double bandwidth_pcm;
  unsigned downsample;
  int us_version;
  unsigned table_size;
  unsigned if_filter_order;
  /* How the IF FIR adds up an output's taps.  FMD_FIR_SEQUENTIAL (0, the default and the only mode
   * under the parity contract): one lane per output, taps in the reference's order
   * (DownConvert.cpp:117-121) -- bit-identical results.  FMD_FIR_SHUFFLE_PARITY_WAIVED: the sum split
   * over four lanes and combined with wavefront shuffles (the reduction BASELINE's north star names):
   * a different order of float additions.  Measured on BASELINE config 2 (6 s): audio 1.2e-5 RMS from
   * the reference (worst block 3.5e-5) -- ABOVE the 1e-5 RMS the contract allows -- and 3x slower, so
   * whoever asks for it says in the value itself that parity is waived; a plain 1 is refused.
   * Headline window layout only (odd downsample, power-of-two tuner table), other geometries ignore it.
   * FMD_FIR_FMA_PARITY_WAIVED: the reference's tap order, every multiply-add fused (v_pk_fma_f32: one rounding
   * per tap instead of two) in the IF FIR and in the two fractional resamplers (DownConvert.cpp:117-121,
   * 203-232) -- what an x86 build of the reference with -march=native does to the same loops (BASELINE.md
   * section 2: "output bits change").  Not bit-identical, so it too has to be asked for by name (a plain 2 is
   * refused); it exists to put a price on bit-exactness (docs/MEASUREMENTS.md: audio RMS distance, joules per
   * call, MS/s).  Reference geometry only (88 taps, downsample 11); refused elsewhere. */
  int fir_reduction;
} fmd_params;

/* Upward callbacks = the three cRadioReceiver members the RDS group decoder calls
 * (RadioReceiver.h:77,80,115; called from RDSGroupDecoder.cpp:403,405,981,990).  Invoked on
 * the calling thread from inside fmd_process_stream / fmd_batch_process_host.  A NULL entry
 * behaves like the reference with no dialog open (frames accepted, name accepted, inactive).
 * frame = ADD(2) SQC MFL payload CRC16(2), unstuffed, valid only during the call. */
typedef struct fmd_callbacks
{
  int (*add_uecp_frame)(void* user, unsigned channel, const uint8_t* frame, unsigned len);
  int (*set_channel_name)(void* user, unsigned channel, const char name[9]);
  int (*is_setting_active)(void* user, unsigned channel);
} fmd_callbacks;

/* Getters of cFmDecoder (FmDecode.h:140-165) */
typedef struct fmd_status
{
  int stereo_detected;   /* StereoDetected()    */
  float tuning_offset;   /* GetTuningOffset()   */
  float interface_level; /* GetInterfaceLevel() */
  float baseband_level;  /* GetBasebandLevel()  */
  float pilot_level;     /* GetPilotLevel()     */
  int rds_state;         /* 0 bit sync, 1 block sync, 2 group decode, 3 group resync */
} fmd_status;

/* One RDS group = the uint16_t[4] the signal processor hands to the group decoder
 * (RDSProcess.cpp:312,355): the bit-exact parity checkpoint. */
typedef struct fmd_rds_group
{
  uint32_t channel;
  uint32_t call_index; /* 1-based index of the process call that completed the group */
  uint16_t blocks[4];
} fmd_rds_group;

/* ---- single decoder: the cFmDecoder surface --------------------------------------- */
typedef struct fmd_decoder fmd_decoder;

/* cFmDecoder::cFmDecoder (FmDecode.cpp:237-314) */
int fmd_create(const fmd_params* params, const fmd_callbacks* cb, void* user, fmd_decoder** out);
/* cFmDecoder::~cFmDecoder (FmDecode.cpp:316-324) */
void fmd_destroy(fmd_decoder* d);
/* cFmDecoder::Reset (FmDecode.cpp:326-338) */
int fmd_reset(fmd_decoder* d);
/* cFmDecoder::ProcessStream (FmDecode.cpp:417-502): iq = samples complex<float> (host),
 * audio = caller buffer of samples*2 floats (RadioReceiver.cpp:519-520); returns the number
 * of floats written (2 per audio frame) or a negative error. */
int fmd_process_stream(fmd_decoder* d, const float* iq, unsigned samples, float* audio);
/* cRtlSdrSource::ReadAsyncCB (RTL_SDR_Source.cpp:196-213) + ProcessStream in one call: buf =
 * 2*samples bytes as librtlsdr delivers them (I, Q, I, Q, ...).  Every byte is converted with the
 * reference's float(b / (255.0 / 2.0) - 1.0) inside the IF kernel, so the result equals
 * fmd_process_stream on the converted block; the transfer and the HBM read are 4x smaller. */
int fmd_process_stream_u8(fmd_decoder* d, const uint8_t* buf, unsigned samples, float* audio);
/* The same for any input format (FMD_IQ_*): iq = samples (I, Q) pairs of that format. */
int fmd_process_stream_fmt(fmd_decoder* d, const void* iq, int format, unsigned samples, float* audio);
/* ... and any output format (FMD_PCM_*): audio = caller buffer of samples*2 elements of that format; returns the
 * number of samples written (2 per audio frame) or a negative error. */
int fmd_process_stream_pcm(fmd_decoder* d, const void* iq, int iq_format, unsigned samples, void* audio,
                           int pcm_format);
/* ... and the multiplex beside it (FMD_MPX_*): mpx = caller buffer of `samples` elements of mpx_format (any
 * alignment), *mpx_samples = how many were written.  mpx == NULL: fmd_process_stream_pcm. */
int fmd_process_stream_mpx(fmd_decoder* d, const void* iq, int iq_format, unsigned samples, void* audio,
                           int pcm_format, void* mpx, int mpx_format, unsigned* mpx_samples);
/* ... or the mono feed beside the audio (FMD_FEED_*; turned on with fmd_batch_set_feed(fmd_decoder_batch(d), 2 or
 * 3)): feed = caller buffer of fmd_batch_max_feed_samples elements of feed_format (any alignment), *feed_samples =
 * how many were written.  feed == NULL: fmd_process_stream_pcm.  A feed pointer while the feed is off:
 * FMD_ERR_STATE. */
int fmd_process_stream_feed(fmd_decoder* d, const void* iq, int iq_format, unsigned samples, void* audio,
                            int pcm_format, void* feed, int feed_format, unsigned* feed_samples);
int fmd_get_status(fmd_decoder* d, fmd_status* st);
/* The one-channel batch behind a decoder: for the profiling / development calls below (fmd_batch_set_
 * profiling, fmd_batch_get_stage_ms, fmd_batch_debug_*); not for processing (the decoder owns it). */
struct fmd_batch;
struct fmd_batch* fmd_decoder_batch(fmd_decoder* d);

/* ---- batch of independent channels on one GPU -------------------------------------- */
typedef struct fmd_batch fmd_batch;

/* Non-finite and denormal input.  Float IQ from a host or a damaged file may hold infinities, NaNs, values that overflow
 * inside the IF filter's sum, and denormals.  A channel decodes such input as the reference's decoder decodes it: every
 * output -- stage taps, audio in either format, multiplex, feed and channel IQ rows, the getters, RDS groups, block
 * records and counters -- equals the reference's, finite values, infinities (with their sign), zeros (with theirs) and
 * denormals bit for bit, and NaN where the reference has a NaN (sign and payload of a NaN are the processor's: an
 * invalid operation gives 0xFFC00000 on x86 and 0x7FC00000 here).  Nothing is flushed, clamped or skipped, and no input
 * value faults: the one address formed from a sample value, the serial stage's sine table offset, reads 0 beyond the
 * table for a NaN phase, whose result is NaN anyway.
 *  - Only the channels that read a capture are touched by what it holds: every other channel keeps the bits of the
 *    same run without it, whatever lanes, waves and workgroups the two share.
 *  - As in the reference, a decoder that has met a NaN stays poisoned: the FM PLL's state is NaN from the first
 *    non-finite IF sample on, and with it baseband, audio and the RDS chain.  cFmDecoder::Reset does not clear all of
 *    it, so neither do fmd_reset, fmd_batch_reset and fmd_batch_reset_channels: behind a reset the baseband is finite at
 *    once, the resamplers and the RDS low-pass give NaN for the length of their histories, and the RDS PLL, matched
 *    filter and bit recovery and the audio stay NaN for good (recursive state that Reset leaves behind).
 *    fmd_batch_switch_captures carries the whole state, so a switch to a clean capture does not revive a slot either.
 *  - What revives a slot is a new decoder: fmd_batch_retune_channels[_to] (also to the shift the slot has), or
 *    fmd_batch_import_channels / fmd_batch_load_state of a decoder that was clean.  An exported, saved or moved
 *    decoder is the decoder it was, NaNs included.
 *  - FMD_PCM_S16, FMD_MPX_S16, FMD_FEED_S16 and FMD_CIQ_S16 give 0 for a NaN and saturate an infinity;
 *    fmd_batch_read_pcm_clipped counts the latter and not the former.  The audio meter is NaN after a call with a NaN.
 *  - The receiver (fmd_receiver_signal_status, fmd_receiver_pvr_signal_status) is outside this statement: like
 *    cRadioReceiver::GetSignalStatus it converts a float level to int, which is undefined for NaN in the reference.
 *  - The band scan: see fmd_scan_finish_*.
 * tests/test_gpu_poison.py holds every one of these against the CPU oracle, lane by lane. */

/* All channels share params (same geometry); tuning_shifts (optional, n_channels entries)
 * overrides the cFineTuner shift per channel (config 3: many stations from one capture),
 * NULL derives it from params->tuning_offset like FmDecode.cpp:250.  device = HIP ordinal. */
int fmd_batch_create(const fmd_params* params, unsigned n_channels, const int* tuning_shifts,
                     int device, const fmd_callbacks* cb, void* user, fmd_batch** out);
void fmd_batch_destroy(fmd_batch* b);
int fmd_batch_reset(fmd_batch* b);

/* upper bounds for sizing caller buffers */
unsigned fmd_batch_channels(const fmd_batch* b);
/* How many of the batch's internal streams share a hardware queue with another stream of the process
 * (found by a probe when the batch was created; 0 = every chain of a call can overlap the others as measured).
 * HIP maps streams onto GPU_MAX_HW_QUEUES queues -- 4 unless the host process sets that variable before the
 * runtime initialises; the library reads no environment variable.  When the number is not 0, fmd_batch_create
 * still returns FMD_OK and leaves a sentence saying so in fmd_last_error(). */
int fmd_batch_streams_sharing_queue(const fmd_batch* b);
/* smallest `samples` a process call of this batch accepts (see FMD_MIN_BLOCK) */
unsigned fmd_batch_min_samples(const fmd_batch* b);
/* The baseband lengths M a call with channel IQ rows as input (FMD_IN_CIQ_*) may have: [*min, *max], multiples of
 * *multiple (any pointer may be NULL).  FMD_ERR_ARG for a null batch. */
int fmd_batch_baseband_limits(const fmd_batch* b, unsigned* min, unsigned* max, unsigned* multiple);
unsigned fmd_batch_max_audio_floats(const fmd_batch* b, unsigned samples);
/* multiplex samples per channel a call of `samples` delivers at most (see FMD_MPX_*): the bound for sizing rows */
unsigned fmd_batch_max_mpx_samples(const fmd_batch* b, unsigned samples);
/* multiplex samples per second: sample_rate_if / downsample */
double fmd_batch_mpx_rate(const fmd_batch* b);

/* The feed's divisor (FMD_FEED_*).  2 or 3 turns the feed on: the taps are designed and uploaded, the scratch of mono
 * frames ((taps - 1 + the longest call's frames) x channels floats per 8192 channels) is allocated, the history is
 * zeroed and g = 0 -- also when the feed was already on, with the same divisor or the other.  0 turns it off and frees
 * the scratch.  Anything else is FMD_ERR_ARG (any other divisor would be cut off by the design's cap of 75 taps:
 * -32 dB at 4), as are a null or failed batch.  It applies in front of the next call submitted, like
 * fmd_batch_set_rds_blocks; it is a setup call and it allocates: it WAITS for the calls in flight. */
int fmd_batch_set_feed(fmd_batch* b, int divisor);
/* the divisor (0: off), or a negative error */
int fmd_batch_get_feed(const fmd_batch* b);
/* feed samples per second: sample_rate_pcm / divisor; 0 while the feed is off */
double fmd_batch_feed_rate(const fmd_batch* b);
/* feed samples per channel a call of `samples` delivers at most: the bound for sizing rows; 0 while the feed is off */
unsigned fmd_batch_max_feed_samples(const fmd_batch* b, unsigned samples);
/* the taps in use into out[0 .. cap); returns their number (0 while the feed is off) */
int fmd_batch_get_feed_taps(const fmd_batch* b, float* out, unsigned cap);

/* Device-resident call, asynchronous on `stream` (hipStream_t, NULL = default stream).
 *  d_iq            complex<float> IQ in HBM; channel c starts at d_iq + 2*c*iq_channel_stride
 *                  floats; iq_channel_stride == 0 means one shared capture for all channels.
 *  d_audio         channel c's interleaved L/R floats at d_audio + c*audio_channel_stride.
 *  out_floats      (host, optional) floats written per channel -- the same for every
 *                  channel of a batch, known when the call returns.
 * RDS groups produced by the call stay queued on the device until fmd_batch_collect_rds /
 * fmd_batch_export_rds_device drains them.  A call appends to one of 8 queues in rotation (call index
 * mod 8), each holding max(4096, 8 x channels) groups; a caller that never drains loses the groups
 * beyond that (FMD_WARN_RDS_LOST) and nothing else. */
int fmd_batch_process_device(fmd_batch* b, const float* d_iq, size_t iq_channel_stride,
                             unsigned samples, float* d_audio, size_t audio_channel_stride,
                             unsigned* out_floats, void* stream);

/* Same with RTL-SDR byte pairs as input (see fmd_process_stream_u8): channel c starts at
 * d_iq_u8 + 2*c*iq_channel_stride bytes.  Both entry points need the pointer and the channel
 * stride to be multiples of two IQ samples (16 bytes of float IQ, 4 bytes of byte IQ). */
int fmd_batch_process_device_u8(fmd_batch* b, const uint8_t* d_iq_u8, size_t iq_channel_stride,
                                unsigned samples, float* d_audio, size_t audio_channel_stride,
                                unsigned* out_floats, void* stream);

/* Same for any input format (FMD_IQ_*): channel c starts iq_channel_stride IQ samples of that format behind
 * channel c - 1.  Pointer and stride: multiples of two IQ samples (see FMD_IQ_*). */
int fmd_batch_process_device_fmt(fmd_batch* b, const void* d_iq, int format, size_t iq_channel_stride,
                                 unsigned samples, float* d_audio, size_t audio_channel_stride,
                                 unsigned* out_floats, void* stream);

/* Same for any output format (FMD_PCM_*): channel c's interleaved L/R samples start audio_channel_stride elements of
 * that format behind channel c - 1's, and *out_samples counts elements of it (fmd_batch_max_audio_floats is the
 * bound for both formats: it is a sample count).  FMD_PCM_S16: d_audio must be 16-byte aligned and
 * audio_channel_stride a multiple of 8 elements (a lane stores four frames at a time), else FMD_ERR_ARG; nothing is
 * written behind a row's out_samples elements. */
int fmd_batch_process_device_pcm(fmd_batch* b, const void* d_iq, int iq_format, size_t iq_channel_stride,
                                 unsigned samples, void* d_audio, int pcm_format, size_t audio_channel_stride,
                                 unsigned* out_samples, void* stream);

/* The _pcm call with every channel's demodulated multiplex beside the audio (FMD_MPX_*): channel c's row starts
 * mpx_channel_stride elements of mpx_format behind channel c - 1's and takes *out_mpx_samples = M samples.
 * d_mpx == NULL makes it exactly the _pcm call (*out_mpx_samples = 0).  d_mpx must be 16-byte aligned and
 * mpx_channel_stride a multiple of 4 elements (FMD_MPX_F32) or 8 (FMD_MPX_S16) and >= M
 * (fmd_batch_max_mpx_samples(b, samples) always is), else FMD_ERR_ARG and the batch is exactly as it was; nothing is
 * written behind a row's M elements.  The rows are written by a transposing kernel behind the call's serial stage,
 * beside the resampler.  Like d_audio's rows they are complete when the call is -- in the order of `stream` with
 * concurrency 0 and 1, behind the fmd_batch_wait[_lagged] that covers the call with concurrency 2: a caller with
 * calls in flight gives each of them rows of its own and does not read them before that wait. */
int fmd_batch_process_device_mpx(fmd_batch* b, const void* d_iq, int iq_format, size_t iq_channel_stride,
                                 unsigned samples, void* d_audio, int pcm_format, size_t audio_channel_stride,
                                 unsigned* out_samples, void* d_mpx, int mpx_format, size_t mpx_channel_stride,
                                 unsigned* out_mpx_samples, void* stream);

/* The _mpx call with every channel's mono feed beside audio and multiplex (FMD_FEED_*): channel c's row starts
 * feed_channel_stride elements of feed_format behind channel c - 1's and takes *out_feed_samples samples.
 * d_feed == NULL makes it exactly the _mpx call: *out_feed_samples = 0, the feed's frame count g does not advance, and
 * the call launches what the _mpx call launches -- the feed is the concatenation of the calls that asked for it, such a
 * call is a splice in it, not a gap of zeros.  A non-NULL d_feed while the feed is off is FMD_ERR_STATE.  d_feed must
 * be 16-byte aligned and feed_channel_stride a multiple of 4 elements (FMD_FEED_F32) or 8 (FMD_FEED_S16) and >= the
 * call's sample count (fmd_batch_max_feed_samples(b, samples), rounded up, always is), else FMD_ERR_ARG and the batch
 * is exactly as it was; a feed_format outside 0..1 is refused first.  Nothing is written behind a row's samples.  The
 * rows are written behind the call's audio tail, in front of its status record: like d_audio's rows they are complete
 * when the call is (see fmd_batch_process_device_mpx for what that means with concurrency 2). */
int fmd_batch_process_device_feed(fmd_batch* b, const void* d_iq, int iq_format, size_t iq_channel_stride,
                                  unsigned samples, void* d_audio, int pcm_format, size_t audio_channel_stride,
                                  unsigned* out_samples, void* d_mpx, int mpx_format, size_t mpx_channel_stride,
                                  unsigned* out_mpx_samples, void* d_feed, int feed_format, size_t feed_channel_stride,
                                  unsigned* out_feed_samples, void* stream);

/* Host-buffer call: copies in, runs fmd_batch_process_device, copies audio out, collects RDS
 * groups and runs the UECP group decoder (callbacks fire here).  Synchronous.  Returns FMD_OK, a
 * negative error, or FMD_WARN_RDS_LOST (once) when groups were dropped because a queue was full:
 * audio and channel state are intact. */
int fmd_batch_process_host(fmd_batch* b, const float* iq, size_t iq_channel_stride,
                           unsigned samples, float* audio, size_t audio_channel_stride,
                           unsigned* out_floats);
int fmd_batch_process_host_u8(fmd_batch* b, const uint8_t* iq_u8, size_t iq_channel_stride,
                              unsigned samples, float* audio, size_t audio_channel_stride,
                              unsigned* out_floats);
int fmd_batch_process_host_fmt(fmd_batch* b, const void* iq, int format, size_t iq_channel_stride,
                               unsigned samples, float* audio, size_t audio_channel_stride,
                               unsigned* out_floats);
/* Any output format (FMD_PCM_*); any stride and alignment of `audio` (rows are copied): FMD_PCM_S16 brings half the
 * bytes back from the device. */
int fmd_batch_process_host_pcm(fmd_batch* b, const void* iq, int iq_format, size_t iq_channel_stride,
                               unsigned samples, void* audio, int pcm_format, size_t audio_channel_stride,
                               unsigned* out_samples);

/* ... and the multiplex (FMD_MPX_*) into host rows of any stride >= M and any alignment (rows are copied through a
 * device staging buffer that is sized on first use); mpx == NULL: fmd_batch_process_host_pcm. */
int fmd_batch_process_host_mpx(fmd_batch* b, const void* iq, int iq_format, size_t iq_channel_stride,
                               unsigned samples, void* audio, int pcm_format, size_t audio_channel_stride,
                               unsigned* out_samples, void* mpx, int mpx_format, size_t mpx_channel_stride,
                               unsigned* out_mpx_samples);

/* ... and the feed (FMD_FEED_*) into host rows of any stride >= the call's sample count and any alignment (rows are
 * copied through a device staging buffer that is sized on first use); feed == NULL: fmd_batch_process_host_mpx. */
int fmd_batch_process_host_feed(fmd_batch* b, const void* iq, int iq_format, size_t iq_channel_stride,
                                unsigned samples, void* audio, int pcm_format, size_t audio_channel_stride,
                                unsigned* out_samples, void* mpx, int mpx_format, size_t mpx_channel_stride,
                                unsigned* out_mpx_samples, void* feed, int feed_format, size_t feed_channel_stride,
                                unsigned* out_feed_samples);

/* Which channels deliver rows.  By default a call writes one audio row and -- where it is
 * asked for the multiplex -- one multiplex row per channel.  From the next call submitted on,
 * fmd_batch_select_audio(b, channels, n) makes row i of d_audio channel channels[i]'s: the call writes exactly n
 * rows, in the order of the list, and nothing else into d_audio.  fmd_batch_select_mpx does the same for d_mpx.
 * channels == NULL restores one row per channel (then n is ignored); a list with n == 0 delivers no rows of that
 * output: d_audio may then be NULL in the device calls and `audio` in the host calls, and a call with an empty
 * multiplex selection is the call with d_mpx == NULL (*out_mpx_samples = 0).  The two selections are independent of
 * each other and of the formats, which stay arguments of the call; *out_samples and *out_mpx_samples are what they
 * were.  The pointer and stride rules hold per row as before (FMD_PCM_S16: 16-byte aligned, stride a multiple of 8;
 * multiplex: 16-byte aligned, stride a multiple of 4 / 8 and >= M); a NULL d_audio with rows to write is
 * FMD_ERR_ARG.  The host calls (fmd_batch_process_host_*) copy back the selected rows only: `audio` / `mpx` hold n
 * rows.
 *
 * Nothing else moves: channel state, status records, the audio meter, RDS groups and the group decoders of every
 * channel, selected or not, keep the bits of the same call without a selection -- an unselected channel's audio tail
 * runs, only its stores and the 16-bit conversion are left out.  fmd_batch_read_pcm_clipped therefore counts
 * delivered samples only (as FMD_PCM_F32 calls add nothing).
 *
 * A selection is applied in front of the next call like fmd_batch_switch_captures: nothing waits, the device is not
 * drained, and calls already submitted (also those in flight under concurrency 2) keep the selection they were
 * submitted with.  It belongs to the slot: resets, retunes, capture switches and imports leave it, the row delivers
 * the decoder the slot now is; it is no part of a state blob and fmd_batch_load_state does not touch it.  Lists hold
 * global channel numbers, also above 8192 channels.
 *
 * FMD_ERR_ARG, the batch as it was: a null batch (no device call is made), a channel out of range or listed twice, a
 * list with n above the channel count, a failed batch.  FMD_ERR_STATE: the batch behind an fmd_decoder
 * (fmd_decoder_batch), whose output the decoder owns.
 *
 * fmd_batch_get_audio_selection / _mpx_selection: the channels of the rows the next call writes into out[0 .. cap),
 * returns their number (the channel count and 0, 1, 2, ... without a selection). */
int fmd_batch_select_audio(fmd_batch* b, const unsigned* channels, unsigned n);
int fmd_batch_select_mpx(fmd_batch* b, const unsigned* channels, unsigned n);
int fmd_batch_get_audio_selection(fmd_batch* b, unsigned* out, unsigned cap);
int fmd_batch_get_mpx_selection(fmd_batch* b, unsigned* out, unsigned cap);
/* The same for the feed rows (d_feed / feed), with fmd_batch_select_mpx's semantics word for word: applied in front
 * of the next call submitted, nothing waits, calls in flight keep the selection they were submitted with; global
 * channel numbers, also above 8192 channels; channels == NULL restores one row per channel.  A list with n == 0 makes
 * the call a call with d_feed == NULL (*out_feed_samples = 0, nothing is written) EXCEPT that the feed's frame count g
 * advances and the history is kept: d_feed must still be a non-NULL, aligned pointer for the call to count as one that
 * asked for the feed.  The scratch rows of EVERY channel are written whatever the selection: a channel selected later
 * has its true history.  The same errors as above. */
int fmd_batch_select_feed(fmd_batch* b, const unsigned* channels, unsigned n);
int fmd_batch_get_feed_selection(fmd_batch* b, unsigned* out, unsigned cap);

/* A process call as one record: the input, one fmd_rows per output, the stream.  It is what
 * the positional entry points above build internally; the channel IQ (FMD_CIQ_*) is reachable only through it.
 *   fmd_rows   p       the output's rows (device pointer in the device call, host pointer in the others); NULL: the
 *                      output is not delivered, and the call is the call of the entry point without that argument
 *              format  FMD_PCM_* (audio), FMD_MPX_* (mpx), FMD_FEED_* (feed), FMD_CIQ_* (ciq)
 *              stride  elements of the format between the rows (ciq: complex samples)
 *              count   (host, optional) elements per row the call wrote (ciq: complex samples)
 *   fmd_call   size    sizeof(fmd_call): anything else is FMD_ERR_ARG (a record of another version of this header)
 *              iq, iq_format, iq_channel_stride, samples: as in fmd_batch_process_device_pcm; or channel IQ rows
 *                      as the input, FMD_IN_CIQ_* (see there: stride in complex samples, samples = M)
 *              stream  hipStream_t of the device call, NULL = default stream; ignored by the other two
 * A record with ciq.p == NULL is fmd_batch_process_device_feed / _host_feed / fmd_process_stream_feed with the same
 * arguments: the same refusals in the same order, the same bits, the same launches, events and allocations.
 * fmd_process_stream_call returns the audio's length like fmd_process_stream_pcm and ignores strides and stream; any
 * of its outputs may be asked for together.
 *
 * ciq: channel c's row starts ciq.stride complex samples behind channel c - 1's and takes *ciq.count = M samples.
 * Device call: ciq.p must be 16-byte aligned and ciq.stride a multiple of 2 samples (FMD_CIQ_F32) or 4
 * (FMD_CIQ_S16) and >= M (fmd_batch_max_mpx_samples(b, samples), rounded up, always is), else FMD_ERR_ARG and the
 * batch is exactly as it was; a ciq.format outside 0..1 is refused before anything else is looked at.  Nothing is
 * written at or behind sample M of a row and nothing for channels the batch does not have.  Host call and decoder:
 * rows of any stride >= M and any alignment, through a device staging buffer sized on first use.  The rows are written
 * by a copying kernel right behind the call's IF stage, on that stage's stream: like d_audio's rows they are complete
 * when the call is, and the call's input buffer counts as free behind them (see fmd_batch_process_device_mpx for what that means with concurrency 2). */
typedef struct fmd_rows
{
  void* p;
  int format;
  size_t stride;
  unsigned* count;
} fmd_rows;
typedef struct fmd_call
{
  size_t size;
  const void* iq;
  int iq_format;
  size_t iq_channel_stride;
  unsigned samples;
  fmd_rows audio, mpx, feed, ciq;
  void* stream;
} fmd_call;
int fmd_batch_process_device_call(fmd_batch* b, const fmd_call* call);
int fmd_batch_process_host_call(fmd_batch* b, const fmd_call* call);
int fmd_process_stream_call(fmd_decoder* d, const fmd_call* call);
/* Which channels deliver channel IQ rows (ciq), with fmd_batch_select_mpx's semantics word for word: applied in front
 * of the next call submitted, nothing waits, calls in flight keep the selection they were submitted with; global
 * channel numbers, also above 8192 channels; channels == NULL restores one row per channel; a list with n == 0 makes
 * the call a call with ciq.p == NULL (*ciq.count = 0); no part of a state blob; FMD_ERR_STATE on the batch behind an
 * fmd_decoder.  The same errors as above. */
int fmd_batch_select_ciq(fmd_batch* b, const unsigned* channels, unsigned n);
int fmd_batch_get_ciq_selection(fmd_batch* b, unsigned* out, unsigned cap);

/* out[i] = the number of audio samples of channel first_channel + i (L and R counted separately) that FMD_PCM_S16
 * calls have saturated since the batch was created: samples whose rounded value lay outside [-32768, 32767] and was
 * clamped (NaN, which gives 0, is not one).  FMD_PCM_F32 calls add nothing.  Like the audio meter it belongs to the
 * output, not to the decoder: fmd_batch_reset, fmd_batch_reset_channels, retunes and capture switches leave it.
 * Synchronous: waits for every call of this batch submitted so far (like the host-buffer call, through the null
 * stream).  A single decoder: through fmd_decoder_batch. */
int fmd_batch_read_pcm_clipped(fmd_batch* b, unsigned first_channel, unsigned n, uint64_t* out);

/* ---- Every RDS block decision, and per-channel reception counters ----
 *
 * RDS leaves a batch as whole groups: four blocks in a row that passed.  The block observation delivers what the
 * synchroniser knows besides -- every 26-bit block it tested, against which offset word, whether it passed clean,
 * was repaired or failed, and when block sync was found, confirmed and lost -- as records, and as eight counters per
 * channel (the block error rate is failed / blocks).  Every value is an integer the reference's own state machine
 * computes (cRDSRxSignalProcessor::ProcessNewRdsBit / CheckBlock, RDSProcess.cpp:272-431); the decoder itself is
 * untouched: audio, groups and status are bit for bit those of a batch that never enabled it.
 *
 * Events.  Every ProcessNewRdsBit: bits++.
 *   BITSYNC (:277-286), whenever CheckBlock(A, no FEC) returns 0: a record (state 0, position 0, status 0,
 *     corrected 0); candidates++.
 *   BLOCKSYNC / GROUPDECODE (:288-359), each time the bit position reaches 26: a record; blocks++.  position is the
 *     entry of BLK_OFFSET_TBL[m_CurrentBlock + m_BGroupOffset] tested: 0 A, 1 B, 2 C, 3 D, 4 C' (entries 4, 5, 7 of
 *     the table are A, B, D again, entry 6 is C').  status 0: the syndrome was zero before the error correction; 1:
 *     non-zero before and zero after it (only GROUPDECODE corrects), corrected++; 2: CheckBlock returned non-zero,
 *     failed++ -- the flips stay applied, as in the reference: `word` and `corrected` say so.  sync_acquired++ when a
 *     state-1 record at D passes, sync_lost++ when a state-2 record fails.
 *   Every DecodeRDS (a group delivered): groups++.
 *   GROUPRESYNC cannot be reached with the reference's BLOCK_ERROR_LIMIT 0; a block boundary passed in it writes and
 *     counts nothing.
 * The counters, and with them bit_index, advance only in calls submitted in mode >= 1.  They belong to the
 * observation of a slot like the clip counter, not to the decoder: fmd_batch_reset, fmd_batch_reset_channels,
 * retunes, capture switches, fmd_batch_load_state and fmd_batch_import_channels restart the machine where they always
 * did and leave the counters alone.  Counters, mode and queues are no part of a state blob (its record format is
 * unchanged). */
typedef struct fmd_rds_block { /* 24 bytes */
  uint32_t channel;
  uint32_t call_index; /* 1-based, as in fmd_rds_group */
  uint32_t bit_index;  /* the channel's `bits` counter after this block's last bit */
  uint32_t raw;        /* low 26 bits of m_InBitStream BEFORE CheckBlock */
  uint16_t word;       /* (m_InBitStream AFTER CheckBlock >> 10) & 0xFFFF */
  uint16_t sample;     /* index in the call's RDS-rate row where the slicer fired for the last bit */
  uint8_t position;    /* offset word tested: 0 A, 1 B, 2 C, 3 D, 4 C' */
  uint8_t status;      /* 0 clean, 1 corrected, 2 failed */
  uint8_t state;       /* machine state BEFORE the check: 0 BITSYNC, 1 BLOCKSYNC, 2 GROUPDECODE */
  uint8_t corrected;   /* bits the Meggitt loop flipped (the reference's correctedbits), failed blocks included */
} fmd_rds_block;

typedef struct fmd_rds_quality { /* 32 bytes, all modulo 2^32 */
  uint32_t bits, candidates, blocks, corrected, failed, sync_acquired, sync_lost, groups;
} fmd_rds_quality;

#define FMD_RDS_BLOCKS_OFF 0
#define FMD_RDS_BLOCKS_COUNT 1  /* counters only */
#define FMD_RDS_BLOCKS_RECORD 2 /* counters + records */
/* The mode of every call submitted from now on; it travels with the call like the formats: nothing waits, calls in
 * flight keep the mode they were submitted with.  A mode-0 call launches what a batch without this launches.
 * queue_records: the record capacity of each of the per-call block queues, 0 = max(8192, 4 * channels) (a shell: per
 * sub-batch); fixed by the first call that enables mode 2, which allocates the queues -- a later different non-zero
 * value is refused. */
int fmd_batch_set_rds_blocks(fmd_batch* b, int mode, unsigned queue_records);
int fmd_batch_get_rds_blocks(const fmd_batch* b); /* the mode, or a negative error */
/* Like fmd_batch_collect_rds_lagged, with bookkeeping of its own: the two drains are independent and either may be
 * called at any cadence.  Copies the block records of the calls at least `lag` (0..4) calls old to `out`, sorted by
 * (call_index, channel, bit_index -- compared wrapping), waits for `stream`; returns their number (<= cap).  Records
 * that did not fit a call's queue, or `out`, are dropped and added to *lost (may be null); no warning flag is touched
 * and the counters never lose anything.  A call's queue is used again eight calls later: records left in it that
 * long come with the later call's, once that call is `lag` calls old (collect at least every eight calls and `lag`
 * means what it says).  fmd_batch_load_state drops queued records, as it drops queued groups. */
int fmd_batch_collect_rds_blocks(fmd_batch* b, fmd_rds_block* out, unsigned cap, int lag, void* stream,
                                 unsigned* lost);
/* The counters of channels [first_channel, first_channel + n).  Synchronous, like fmd_batch_read_pcm_clipped. */
int fmd_batch_read_rds_quality(fmd_batch* b, unsigned first_channel, unsigned n, fmd_rds_quality* out);

/* ---- ITU-R BS.1770 loudness blocks of every channel ----
 *
 * Loudness logging (EBU R 128: momentary, short-term, integrated) needs both audio channels at the PCM rate through
 * the K-weighting filter.  The audio tail has them in registers; with the meter on it also runs the filter and leaves
 * one 16-byte record per channel and block (100 ms by default): the block's sums of squares and sample peaks.  What
 * follows is the definition; it is exact -- the device computes these bits, there is no tolerance on its side.
 *
 * Design.  With fs = sample_rate_pcm, two biquads, designed in double and rounded once to float.
 *   Stage 1, high shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196,
 *     K = tan(pi f0 / fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2,
 *     b0 = (Vh + Vb K/Q + K^2)/a0, b1 = 2 (K^2 - Vh)/a0, b2 = (Vh - Vb K/Q + K^2)/a0,
 *     a1 = 2 (K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0.
 *   Stage 2, high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, the same K and a0 formulas,
 *     b = (1, -2, 1), a1 = 2 (K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0.
 *   At 48 000 Hz these are the coefficients printed in BS.1770-4 (to 1e-15).
 * Filter form.  Each stage, for L and R separately, is transposed direct form II in float; every multiply, add and
 * subtract is rounded on its own (no fused multiply-add), in exactly this order:
 *     y  = b0*x + s1
 *     s1 = (b1*x - a1*y) + s2
 *     s2 = b2*x - a2*y
 *   Stage 2 takes stage 1's y.  The input x is the float audio sample of the call, before any PCM conversion: a
 *   FMD_PCM_S16 call and a channel without an audio row are metered like every other.
 * Blocks.  Frames are numbered g = 0, 1, ... over the calls submitted with the meter on.  Block j is frames
 *   [j Bf, (j + 1) Bf), Bf = block_frames.  Its record is { z_l, z_r, peak_l, peak_r }: z = the sum of y2^2 over the
 *   block in frame order in float (acc = acc + y2*y2, both operations rounded); peak = fmaxf(peak, fabsf(x)) of the
 *   unweighted sample, from 0 -- a NaN sample leaves the peak and makes z NaN.  Filter states and partial sums start at
 *   +0 when the meter is first turned on.  Denormals are kept: a station that falls silent decays through them.
 * tests/loud_spec.py restates all of this in numpy.
 *
 * Ownership.  The meter belongs to the slot's output, like the clip counter and the feed: fmd_batch_reset,
 * fmd_batch_reset_channels, retunes, capture switches, fmd_batch_import_channels and fmd_batch_load_state leave its
 * states, sums and frame count alone; no state blob carries it (the blob's record format is unchanged).  Every channel
 * is metered, whatever the audio selection says.
 *
 * Out of scope: loudness range (EBU Tech 3342) and true peak (4x oversampling; peak_l / peak_r are sample peaks). */
typedef struct fmd_loud_block { /* 16 bytes */
  float z_l, z_r, peak_l, peak_r;
} fmd_loud_block;

#define FMD_LOUDNESS_OFF 0
#define FMD_LOUDNESS_ON 1
/* The mode of every call submitted from now on; it travels with the call like fmd_batch_set_rds_blocks' mode: nothing
 * waits, calls in flight keep theirs.  A mode-0 call launches what a batch without this launches, and it is a splice:
 * the meter does not hear it -- g, states and partial sums stand still.  block_frames: 0 = round(fs / 10) (100 ms),
 * else 16 .. 1048576.  ring_blocks: the blocks of history the device keeps per channel, 0 = 64, else 8 .. 4096.  Both
 * are fixed by the first call that turns the meter on, which allocates (48 + 16 ring_blocks bytes per channel); a
 * later different non-zero value is refused (FMD_ERR_ARG). */
int fmd_batch_set_loudness(fmd_batch* b, int mode, unsigned block_frames, unsigned ring_blocks);
int fmd_batch_get_loudness(const fmd_batch* b); /* the mode, or a negative error */
/* Bf: the fixed value, or before the meter was ever on the default it would take. */
unsigned fmd_batch_loudness_block_frames(const fmd_batch* b);
/* out = b0 b1 b2 a1 a2 of stage 1, then of stage 2: the floats the kernels use. */
int fmd_batch_get_loudness_coeffs(const fmd_batch* b, float out[10]);
/* Copies the not-yet-collected blocks completed by calls at least `lag` (0..4) calls old, for channels
 * [first_channel, first_channel + n_channels) -- global numbers, also above 8192 channels -- to out, block-major:
 * out[k * n_channels + i] is block *first_block + k of channel first_channel + i.  Returns the number of blocks
 * (<= cap_blocks); waits for `stream` and for those calls.  All channels of a batch tick alike and the host knows at
 * submission which call completes which blocks: there is one cursor per batch (a collect takes the blocks for the
 * channels it names and moves it), and nothing is read back to find them.
 * The ring holds the last ring_blocks blocks completed by the calls SUBMITTED so far, in flight or not.  Blocks older
 * than that are skipped and counted in *lost (may be null).  None is lost while, at every collect,
 *     (frames of the calls submitted since the last collected block ended) < ring_blocks * Bf,
 * i.e. collect at least once per (ring_blocks - 1) * Bf frames of mode-1 calls, the `lag` newest calls counted in: with
 * the defaults (64 blocks of 100 ms) once per 6.3 s of audio, some 230 calls of 65 536 samples at 2.4 MS/s.
 * A single decoder: through fmd_decoder_batch. */
int fmd_batch_collect_loudness(fmd_batch* b, fmd_loud_block* out, unsigned cap_blocks, unsigned first_channel,
                               unsigned n_channels, int lag, void* stream, uint64_t* first_block, unsigned* lost);
/* Host arithmetic over block records, in double; no device.
 * fmd_loudness_window: -0.691 + 10 log10((sum z_l + sum z_r) / (n block_frames)) over n consecutive blocks of one
 * channel (summed in block order, z_l then z_r of each): n = 4 momentary, n = 30 short-term loudness (LUFS).
 * fmd_loudness_integrated: BS.1770-4 gating over windows of four consecutive blocks stepping by one (75 % overlap):
 * absolute gate at -70 LUFS, relative gate 10 LU under the loudness of the survivors' mean power; -HUGE_VAL when
 * nothing survives or n_blocks < 4.  A window with a NaN block passes no gate. */
double fmd_loudness_window(const fmd_loud_block* blk, unsigned n, unsigned block_frames);
double fmd_loudness_integrated(const fmd_loud_block* blk, unsigned n_blocks, unsigned block_frames);

/* Copies the queued RDS groups (all channels, call order) to `out`, waits for `stream`.
 * Returns the number of groups (<= cap) or a negative error.  When run_group_decoder != 0
 * each group is also fed to that channel's UECP group decoder (callbacks fire).  The return value is
 * a count, so a loss of groups is not reported here: the flag stays for fmd_batch_wait /
 * fmd_batch_take_rds_lost / fmd_batch_process_host. */
int fmd_batch_collect_rds(fmd_batch* b, fmd_rds_group* out, unsigned cap, int run_group_decoder,
                          void* stream);

/* Like fmd_batch_collect_rds, but the `lag` (0..4) newest calls are left alone: only calls at
 * least that old are waited for and their groups drained (use with concurrency 2, where the
 * newest calls are still running). */
int fmd_batch_collect_rds_lagged(fmd_batch* b, fmd_rds_group* out, unsigned cap,
                                 int run_group_decoder, int lag, void* stream);

/* The same drain without a host round trip, for outputs that travel on as device memory (the rank-0
 * gather of a multi-GPU job): the groups of every call at least `lag` calls old are written to
 * d_records (device memory, 16-byte aligned, cap rows of 4 x int32: channel + 1 + channel_offset,
 * call_index, blocks[0] | blocks[1] << 16, blocks[2] | blocks[3] << 16; rows beyond the groups found
 * are zero, so a fixed-size message can be sent as is) by a kernel on `stream`, and those queues
 * are emptied.  Asynchronous; rows are in no particular order.  More groups than `cap` rows: the
 * surplus is lost and FMD_WARN_RDS_LOST is reported once (by a later wait / export call); the batch
 * stays usable.  Use either this or fmd_batch_collect_rds on a batch, not both for the same calls.
 * One stream at a time: concurrent exports of one batch on different streams are not supported. */
int fmd_batch_export_rds_device(fmd_batch* b, int32_t* d_records, unsigned cap, unsigned channel_offset,
                                int lag, void* stream);

/* Several captures in one batch (BASELINE configs[2] scaled out: G captures x k stations each, where config 3
 * as written is one capture x 256): channels [g k, (g + 1) k) all tune capture g -- the only stage that sees the
 * capture is the tuner in front of the IF filter (cFineTuner::Process, FmDecode.cpp:66-82); everything behind it is
 * per channel as ever.  With k > 1 the iq_channel_stride of the process calls is the distance between CAPTURES
 * (G = channels / k input rows instead of one per channel); k = 0 / 1 restores one row per channel.  iq_channel_stride
 * == 0 still means a single capture for the whole batch.  Not while calls are in flight (the device is drained).
 * It is the contiguous case of the capture map below and replaces any map. */
int fmd_batch_set_channels_per_capture(fmd_batch* b, unsigned channels_per_capture);

/* Capture maps: any channel reads any capture, and a running channel moves to another capture at a call boundary
 * with its state carried over -- what the reference's tuner dialog does when it moves the dongle's LO under a
 * cFmDecoder that keeps running (ChannelSettings.cpp:96-147, 280-289).  DESIGN.md section 9.4.
 *
 * fmd_batch_set_capture_map(b, capture_of_channel, n_captures): channel c reads input row capture_of_channel[c];
 * the process calls (float and byte input, device and host entry points) then take n_captures rows,
 * iq_channel_stride apart.  Any map: a capture's channels need not be contiguous nor in one sub-batch.  NULL
 * restores one row per channel; fmd_batch_set_channels_per_capture(b, k) sets the contiguous map c / k and
 * replaces any map.  iq_channel_stride == 0 still means one capture for every channel.  Not while calls are in
 * flight (the device is drained).  FMD_ERR_ARG: a null batch, n_captures == 0 with a map, a capture out of range.
 *
 * fmd_batch_switch_captures(b, channels, captures, n): from the next call submitted, channel channels[i] reads
 * capture captures[i]; nothing else about the channel changes.  The channel decodes bit for bit like the same
 * cFmDecoder whose input stream continues with the new capture's blocks: its IF filter's first outputs mix the old
 * capture's last tuned samples with the new capture's, and its tuner index, PLLs, RDS sync and UECP group decoder
 * carry over, so audio, RDS groups (with their call index), getters, UECP frames and PS name all follow.  The
 * tuner shift stays (the reference never changes a running cFineTuner's; shifts move only through a retune).
 *  - Works on every batch (no opt-in, no twin).  A batch without a map takes the one its channels-per-capture
 *    rule gives (channel c reads capture c / k) and the switch on top of it.
 *  - Nothing waits: a call with switches overlaps the calls before it like any other call.  Calls already
 *    submitted -- also calls in flight under concurrency mode 2 -- keep the old map.
 *  - Several edits of one channel before one call (switches, resets, retunes, retunes to a capture) apply in the
 *    order they were made: the last capture wins.
 *  - FMD_ERR_ARG: a null batch or list (before the HIP runtime is touched), a channel or capture out of range, a
 *    channel listed twice, a failed batch (fmd_last_error says which).  Same threading rule as the process calls.
 *
 * fmd_batch_retune_channels_to(b, channels, shifts, captures, n): fmd_batch_retune_channels plus a capture: from
 * the next call on, channel channels[i] decodes like a decoder created with shifts[i] that received zeros until
 * now, and reads capture captures[i].  Needs fmd_batch_enable_retune (FMD_ERR_STATE otherwise); errors as above.
 *
 * fmd_batch_get_capture_map(b, out, cap): writes the captures the next call reads for the first min(cap, channels)
 * channels and returns the number of input rows the process calls take (n_captures; channels / k without a map). */
int fmd_batch_set_capture_map(fmd_batch* b, const unsigned* capture_of_channel, unsigned n_captures);
int fmd_batch_switch_captures(fmd_batch* b, const unsigned* channels, const unsigned* captures, unsigned n);
int fmd_batch_retune_channels_to(fmd_batch* b, const unsigned* channels, const int* shifts, const unsigned* captures,
                                 unsigned n);
int fmd_batch_get_capture_map(fmd_batch* b, unsigned* out, unsigned cap);
/* Development switch (not for applications): 0 makes the map form of the IF stage walk the channels in channel
 * order instead of sorted by capture (DESIGN.md section 9.4 measures what the sort is worth); 1 (default) back. */
int fmd_batch_debug_capture_walk(fmd_batch* b, int on);

/* Moving single channels of a running batch to another station (the reference's host deletes its cFmDecoder
 * and creates a new one: RadioReceiver.cpp:296-300, 370-374).  All channels of a batch share one clock (tuner
 * index, decimator and resampler phases, ring positions, RDS oscillator), so a channel cannot become a fresh
 * decoder in the middle of a batch; the exact equivalent it becomes is this one:
 *
 * fmd_batch_retune_channels(b, channels, shifts, n): from the next call on, channel channels[i] decodes exactly
 * like a decoder that was created with tuning shift shifts[i] (the cFineTuner shift of fmd_batch_create's
 * tuning_shifts, taken mod table_size like there) when the batch was created, received zero IQ (float zeros) in
 * every call before this one, and every whole-batch fmd_batch_reset the batch received: audio, getters, RDS
 * groups and the UECP group decoder's frames and name, bit for bit.  Retuning a channel to its own shift
 * restarts it on the same station.
 *  - An edit takes effect at the boundary in front of the next call submitted, whatever the entry point (host,
 *    device, float or byte input, shared captures).  Several edits before one call apply in the order they were
 *    made.  Calls already submitted -- also calls in flight under concurrency mode 2 -- are not affected: their
 *    audio, groups and status records are those of the old tuning.
 *  - Nothing is synchronised: the call applies the edits on the device, behind the calls before it (a call
 *    with edits waits for its predecessors to complete instead of overlapping them).
 *  - Groups of calls before the edit go through the channel's old group decoder state, also when they are
 *    collected later; between the last call before the edit and the first behind it the channel gets a new group
 *    decoder, as the new cFmDecoder would bring one: its UECP sequence counter starts at 0 and it reports the PTY
 *    again (a reset, fmd_batch_reset_channels, keeps both, as cFmDecoder::Reset does).
 *    fmd_batch_get_status's tuning_offset is that of the call the snapshot is of.
 *  - FMD_ERR_ARG: a null batch or list, a channel out of range or listed twice, a failed batch (fmd_last_error
 *    says which).  FMD_ERR_STATE: retuning was not enabled.  Same threading rule as the process calls; the
 *    getters stay safe from any thread.
 *
 * fmd_batch_enable_retune(b): the opt-in, only before the first call (FMD_ERR_STATE after it).  It gives the
 * batch a silent twin -- one channel of the same geometry, fed zeros of every call's size on the batch's
 * streams -- whose state a retuned channel takes over.  A batch that never calls it runs
 * exactly as before. */
int fmd_batch_enable_retune(fmd_batch* b);
int fmd_batch_retune_channels(fmd_batch* b, const unsigned* channels, const int* shifts, unsigned n);

/* Resetting single channels of a running batch: the batched form of cFmDecoder::Reset (FmDecode.cpp:326-338),
 * where fmd_batch_reset resets every channel and drains the device.
 *
 * fmd_batch_reset_channels(b, channels, n): from the next call on, channel channels[i] decodes bit for bit like
 * its own decoder that received the same inputs and a cFmDecoder::Reset() between the last call before this one
 * and the next: audio, getters, RDS groups and the UECP group decoder's frames and name.  Channels not listed stay
 * bit-identical to the same run without the call.  Works on every batch (no opt-in).
 *  - An edit takes effect at the boundary in front of the next call submitted, whatever the entry point (host,
 *    device, float or byte input, shared captures, sub-batches).  Edits before one call -- resets and, with
 *    retuning enabled, retunes of the same channels -- apply in the order they were made.  Calls already
 *    submitted -- also calls in flight under concurrency mode 2 -- are not affected.
 *  - Nothing is synchronised: the next call applies the resets on the device, behind the calls before it (a call
 *    with edits waits for its predecessors to complete instead of overlapping them).
 *  - The getters return the newest completed call's record: the first call behind the reset gives the reset
 *    decoder's values.  The receiver's audio meter (fmd_batch_get_audio_level) is not touched, as with
 *    fmd_batch_reset.
 *  - Groups of calls before the reset go through the channel's old group decoder state, also when they are
 *    collected later; the group decoder is reset between the last call before the reset and the first behind it.
 *  - FMD_ERR_ARG: a null batch or list (before the HIP runtime is touched), a channel out of range or listed
 *    twice, a failed batch (fmd_last_error says which).  Same threading rule as the process calls.
 * The RDS low-pass and matched filter of a reset channel start their rings afresh while the batch's run on; the
 * channel keeps its own ring origin for them.  A batch that never calls this runs exactly
 * as before. */
int fmd_batch_reset_channels(fmd_batch* b, const unsigned* channels, unsigned n);

/* Saving and restoring a running batch; moving live channels between batches.
 *
 * A state blob is an opaque host buffer: a header (magic, layout version, fmd_version()'s string, a fingerprint of
 * the geometry -- every field of fmd_params and the designed sizes, not the channel count or the device --, the
 * batch's clock, the channel count, a checksum over everything) and per channel all that makes the next call's
 * outputs what they are: every carried region of the device state in both buffer parities, the ring origins, the
 * tuning shift, the status record the getters read, the audio meter, the clipped-sample counter and the host's UECP
 * group decoder.  A blob is valid for the same build of the library on the same kind of host; anything else is
 * refused.  NOT carried: RDS groups still queued on the device (collect them from the source before or after: they
 * stay collectable there), profiling state, development switches, the concurrency mode, callbacks, a pending
 * groups-lost warning, the output selections (fmd_batch_select_audio / _mpx: they belong to the slot).
 *
 * fmd_batch_state_size(b, n): bytes a blob of n channels takes (n = the batch's channel count: a whole batch, with
 * its silent twin where retuning is enabled); 0 for a null batch.
 *
 * fmd_batch_save_state: synchronous; waits for every call submitted so far (also calls in flight under concurrency
 * mode 2), writes the whole batch -- a shell's sub-batches, the silent twin, the capture map as the next call would
 * read it, the channels per capture and the call index -- and changes nothing in it.  *written (may be null) gets
 * the blob's size, also when cap is too small (FMD_ERR_ARG).  Edits no call has applied yet (a retune, reset,
 * capture switch, import, a new map) give FMD_ERR_STATE.
 *
 * fmd_batch_load_state: synchronous; waits for the destination's calls.  Checks checksum, version, geometry,
 * channel count (FMD_ERR_ARG) and the retune opt-in (FMD_ERR_STATE: the destination must have called
 * fmd_batch_enable_retune exactly if the source had) before touching anything: on a refusal the destination is
 * untouched.  Then the whole state and the clock are replaced; groups still queued in the destination and its
 * pending edits are dropped (no loss flag); a failed batch may be loaded into, which clears the failure.  From the
 * next call on every output -- audio in either format, getters (right after the load: the source's at the save),
 * RDS groups with their call index, UECP frames and PS name, audio meter, clipped counts -- is bit for bit what the
 * source would have produced for the same inputs, whatever the destination's device, concurrency mode or
 * development switches.
 *
 * fmd_batch_export_channels: as save_state (same waiting rule, same format) for the n listed channels, in list
 * order; any channels of any sub-batch, no duplicates; the source is not disturbed.
 *
 * fmd_batch_import_channels: an edit like a retune -- from the next call submitted, slot channels[i] IS the decoder
 * of the blob's record i (the blob holds exactly n records; its source may have had any channel count).  Calls
 * already submitted keep the old occupant; groups of earlier calls still go through the slot's old group decoder.
 * Edits of one slot before one call apply in the order made (import then reset: the reset decoder; reset or retune
 * then import: the import).  The slot keeps its capture assignment (pair the import with
 * fmd_batch_switch_captures) and takes the record's shift.  No opt-in is needed; the host does not wait for the
 * device.  Clock rule: a decoder continues only in a batch whose batch-uniform words (decimator and resampler
 * positions, tuner index, ring phases, buffer parity: the call index mod 4, the RDS oscillator) equal the blob's in
 * front of the batch's next call -- two batches created or loaded alike and fed the same sequence of call sizes
 * always qualify.  A difference, also one of the buffer parity alone, gives FMD_ERR_STATE naming the first
 * differing word; nothing is queued and the batch carries on.  At most eight imports may wait for one call.
 *
 * All: a null argument or a size below a blob's header is FMD_ERR_ARG before the HIP runtime is touched.  Same
 * threading rule as the process calls.  fmd_save_state / fmd_load_state: the one-channel batch behind a decoder.
 * fmd_batch_debug_state_skip (test aid): the loads and imports that follow leave one region out -- 0..7 the regions
 * of fmd_batch_debug_restart_skip, 8 the status record, 9 the group decoder, 10 the audio meter and clip counter;
 * -1 none (the default).  The restored channel is then not exact. */
size_t fmd_batch_state_size(const fmd_batch* b, unsigned n_channels);
int fmd_batch_save_state(fmd_batch* b, void* blob, size_t cap, size_t* written);
int fmd_batch_load_state(fmd_batch* b, const void* blob, size_t size);
int fmd_batch_export_channels(fmd_batch* b, const unsigned* channels, unsigned n, void* blob, size_t cap,
                              size_t* written);
int fmd_batch_import_channels(fmd_batch* b, const unsigned* channels, unsigned n, const void* blob, size_t size);
int fmd_save_state(fmd_decoder* d, void* blob, size_t cap, size_t* written);
int fmd_load_state(fmd_decoder* d, const void* blob, size_t size);
int fmd_batch_debug_state_skip(fmd_batch* b, int region);

/* Internal execution.  A call is four independent kernel chains (FIR -> serial demodulator ->
 * {RDS branch, audio branch}); mode selects where they run:
 *   0  all on the caller's stream, in order
 *   1  on internal streams, the caller's stream is ordered after each call (default; same
 *      observable semantics as 0)
 *   2  on internal streams and the caller's stream is NOT ordered after the call: the FIR of
 *      call k+1 overlaps the serial stages of call k.  The caller must use different audio buffers
 *      for calls in flight, keep d_iq and d_audio valid, and call fmd_batch_wait[_lagged] (or
 *      collect_rds) before consuming outputs (d_mpx's rows of the _mpx call included). */
int fmd_batch_set_concurrency(fmd_batch* b, int mode);
/* Orders `stream` after every call submitted so far (outputs complete, inputs released). */
int fmd_batch_wait(fmd_batch* b, void* stream);
/* lag = 1..4: every call except the newest `lag` ones (whose kernels may still be running: a call is
 * complete about 1.3 periods after its serial stage has started, so a host that must never block
 * consumes outputs two to three calls late). */
int fmd_batch_wait_lagged(fmd_batch* b, int lag, void* stream);
/* 1 if RDS groups were lost since the last report (see FMD_WARN_RDS_LOST; clears the flag), else 0. */
int fmd_batch_take_rds_lost(fmd_batch* b);

/* The getters of cFmDecoder for one channel (FmDecode.h:140-165).  They return the status the
 * newest COMPLETED call left behind (all zero before the first call; Reset zeroes what
 * cFmDecoder::Reset zeroes): the last kernel of every call writes a small record per channel into
 * host-mapped memory, and the getters only read that record -- no device synchronisation, no stream
 * operation, nothing of the batch is modified.  They may be called from any thread at any time,
 * also while another thread is inside a process call on the same batch (Kodi's status thread does
 * that: RadioReceiver.cpp:544-572 against :524).  A record is always one call's values, never a mix
 * of two writes (rds_state, which is no cFmDecoder getter, is a word of its own that the bit recovery
 * updates).  With overlapped calls (concurrency 2) the interface / baseband meters in it may already
 * include the following call. */
int fmd_batch_get_status(fmd_batch* b, unsigned channel, fmd_status* st);
/* index (1-based) of the call whose status the getters return at this moment, 0 = none yet */
int fmd_batch_status_call_index(fmd_batch* b, unsigned channel, uint32_t* call_index);

/* cRadioReceiver's audio level meter over the audio a call produced (RadioReceiver.cpp:526-528,
 * SamplesMeanRMS :584-598): float sums over the interleaved samples of the packet, then
 * level = 0.95 * level + 0.05 * rms.  Computed on the device while the audio is written; `level`
 * starts at 0 when the batch is created and, like m_AudioLevel, is not touched by Reset. */
typedef struct fmd_audio_level
{
  float mean;  /* audio_mean of the last call */
  float rms;   /* audio_rms of the last call  */
  float level; /* m_AudioLevel                */
} fmd_audio_level;
int fmd_batch_get_audio_level(fmd_batch* b, unsigned channel, fmd_audio_level* out);

/* Stage taps for parity tests: copies stage output of the last call for one channel to host.
 * Returns element count (complex counts as one) or negative error. */
enum fmd_tap
{
  FMD_TAP_DEMOD = 0,    /* complex: IF FIR output            */
  FMD_TAP_BASEBAND = 1, /* FM PLL output                     */
  FMD_TAP_PILOT38 = 2,  /* 38 kHz * 2 * baseband             */
  FMD_TAP_MONO_RS = 3,  /* mono resampler output             */
  FMD_TAP_STEREO_RS = 4,/* stereo resampler output           */
  FMD_TAP_RDS_LPF = 5,  /* complex: RDS 75-tap LPF output    */
  FMD_TAP_RDS_PLL = 6,
  FMD_TAP_RDS_MF = 7,
  FMD_TAP_RDS_SYNC = 8
};
int fmd_batch_get_tap(fmd_batch* b, int tap, unsigned channel, float* out, unsigned cap_floats);
/* The three RDS-recurrence taps (PLL, matched filter, bit sync) cost extra stores per sample and
 * are only written while enabled (default off). */
int fmd_batch_set_debug_taps(fmd_batch* b, int enable);

/* Design constants / taps as the host computed them (for parity with the oracle). */
int fmd_batch_get_design(fmd_batch* b, int what, float* out, unsigned cap);
enum fmd_design_item
{
  FMD_DESIGN_IF_TAPS = 0,
  FMD_DESIGN_RS_TAPS = 1,
  FMD_DESIGN_AUDIO_LPF = 2,
  FMD_DESIGN_RDS_LPF = 3,
  FMD_DESIGN_RDS_MF = 4,
  FMD_DESIGN_SCALARS = 5, /* same order as oracle fmo_get_constants */
  FMD_DESIGN_LUT0 = 6     /* channel 0 cFineTuner table, interleaved */
};

/* Device time per stage, measured with HIP events recorded on the call's own stream.
 * level 0 = off, 1 = events around the IF FIR kernel only, 2 = around every stage.  Each call
 * made while profiling is on gets its own event set (no synchronisation inside the calls);
 * fmd_batch_get_stage_ms synchronises the device, writes the AVERAGE ms per stage over those
 * calls (-1 for stages not covered at level 1; index = fmd_stage_name index) and returns the
 * number of calls averaged.  set_profiling restarts the averaging window. */
int fmd_batch_set_profiling(fmd_batch* b, int level);
int fmd_batch_get_stage_ms(fmd_batch* b, float* out, unsigned cap);
const char* fmd_stage_name(unsigned idx);

/* Test aid: evaluates the device build of one math helper of csrc/fmd_math.h on n arguments
 * (host arrays).  what: 0 atan2f table form (a = y, b = x), 1 atan2f literal fdlibm, 2 sin/cos
 * table form (a = phase; out0 = sin, out1 = cos), 3 sin/cos series form, 4 mid-range division
 * a / b, 5 RTL-SDR byte -> float (a = byte value), 6 the RDS PLL's polynomial arctan2, 7 sin/cos of a
 * phase in [0, 8) with the exact float reduction (the serial stage's two NCOs), 8 float -> 16-bit PCM
 * (fmd_f32_to_s16 of a; out0 = the integer as a float), 9 float -> 16-bit multiplex (fmd_f32_to_mpx16 of a, likewise). */
int fmd_debug_math(int what, unsigned n, const float* a, const float* b, float* out0, float* out1);

/* Dev aid, only with FMD_SERIAL_PROBE=1 in the environment at batch creation: per workgroup of the
 * serial stage's last 8 launches, (start, end) on the device's 100 MHz clock and the shader-clock
 * cycles in between (low 40 bits; HW_ID bits 8-15 and XCC_ID above): 8 x (padded channels / 64) records of 3 x int64, launch = call index mod 8,
 * records of workgroups that did not exist stay zero.  Returns the number of records written (0
 * when the probe is off).  Synchronises the device. */
int fmd_batch_debug_serial_probe(fmd_batch* b, long long* out, unsigned cap_workgroups);
/* Dev aid: which internal streams share a hardware queue with the caller's `stream` (bit i: internal stream i waits
 * behind it; bit 8 + i: it waits behind internal stream i; 0 = none).  Drains the device. */
int fmd_batch_debug_stream_conflicts(fmd_batch* b, void* stream);
/* Dev aid (overlapped calls at profiling level 1, whole-CU serial stage): per profiled call when its
 * IF FIR, its serial stage, its audio tail, its half-band chain and its resampler started and ended on
 * the device (the last two only in their large-batch forms), in ms since the first profiled call's FIR
 * started: cap_calls rows of 10 floats (-1 = not recorded).  Returns the number of rows.  Synchronises
 * the device.  What a short run's fill and drain are made of (bench.py prints it with
 * FMD_BENCH_TIMELINE=1). */
int fmd_batch_debug_timeline(fmd_batch* b, float* out, unsigned cap_calls);
/* Dev aid (tools/mpx_bench.py): the first query switches the timing on and returns 0 -- from then on the multiplex
 * writer of the batch's _mpx calls is launched with events of its own at its start and stop; later queries:
 * out[i] = its ms in one of the last 8 such calls.  Returns the number written.  Synchronises the device.  (A batch
 * above 8192 channels: its first sub-batch.) */
int fmd_batch_debug_mpx_ms(fmd_batch* b, float* out, unsigned cap);
/* Test aid: bound (in polls) of the serial stage's LDS hand-off waits for the calls that follow;
 * 0 makes every wait time out at once, which exercises the device-side error path. */
int fmd_batch_debug_set_spin_limit(fmd_batch* b, unsigned limit);
/* Development switches of one batch, by name (the shipped library reads NO environment variable).
 * They select between implementations that give identical results, or add instrumentation; they
 * apply to the calls that follow and may be changed while no call is in flight.  Returns FMD_ERR_ARG
 * for an unknown key.  Keys: see fmd_batch_debug_set in csrc/fmd_batch.hip ("resampler": -1 the
 * library decides, 0 window per wave (k_resample), 1 LDS ring (k_resample_ring) wherever the
 * geometry allows it; ...). */
int fmd_batch_debug_set(fmd_batch* b, const char* key, int value);
/* Where the time of the host-buffer calls (fmd_batch_process_host*, fmd_process_stream*) went since the
 * last query, mean ms per call: out[0] copy of the IQ block to the device, [1] submission of the call's
 * kernels, [2] waiting for them + copy of the audio back, [3] collection of the RDS groups + UECP group
 * decoder callbacks.  Returns the number of calls averaged. */
int fmd_batch_debug_host_ms(fmd_batch* b, float out[4]);
/* Test aid (the mutation test of the restart, tests/test_gpu_retune.py): the restarts of the calls that follow
 * leave out one region of the carried state -- region = its index in kRestartRegions of csrc/fmd_batch.hip (0
 * state, 1 if_hist, 2 br, 3 mix, 4 halfband, 5 rds_lpf, 6 rds_mf, 7 audio_lpf) -- and a retuned channel is no
 * longer exact (the rds_lpf / rds_mf regions include the ring origins).  -1 (the default) leaves nothing out; other
 * values: FMD_ERR_ARG. */
int fmd_batch_debug_restart_skip(fmd_batch* b, int region);
/* Test aid (the teeth test of the single-channel reset, tests/test_gpu_reset_channels.py): on != 0 makes the
 * resets of the calls that follow leave the channels' ring origins at the batch's phase (0), and a reset channel's
 * RDS low-pass and matched filter are no longer exact.  0 (the default) restores the origins. */
int fmd_batch_debug_reset_keep_ring_phase(fmd_batch* b, int on);
/* Test aid (mutation test of the feed's tests): on = 1 leaves out the roll behind every feed call, so the history rows
 * in front of a call's frames stay what they were -- the first feed sample that reaches back over a call boundary is
 * then wrong.  An entry point of its own: the fmd_batch_debug_set key table is held to 14 keys. */
int fmd_batch_debug_feed_skip_roll(fmd_batch* b, int on);
/* Test aid (mutation test of the loudness meter's tests): on = 1 makes every mode-1 call start its block in progress
 * from +0 -- the carried partial sums and peaks are dropped at the call boundary, so exactly the blocks that span one
 * are wrong.  An entry point of its own, like the one above. */
int fmd_batch_debug_loud_skip_carry(fmd_batch* b, int on);
/* Test aid (mutation test of FMD_IN_CIQ_*): the input copy leaves out every row's last tile. */
int fmd_batch_debug_ciq_in_skip_tile(fmd_batch* b, int on);
/* Test aid: out[i] = the host build of FMD_IN_CIQ_S16's conversion of in[i], (float)v * 2^-13; no device is touched. */
int fmd_debug_ciq16_to_f32(const int16_t* in, unsigned n, float* out);

const char* fmd_last_error(void);
const char* fmd_version(void);

/* ---- the stream side of cRadioReceiver around the decoder --------------------------- */
/* What turns blocks of IQ into Kodi demux packets and the signal-status maths on
 * top of the decoder's getters (8(f)-4): cRadioReceiver::OpenLiveStream's stream state
 * (RadioReceiver.cpp:296-349), WriteDataBuffer / EndDataBuffer / SourceGetSamples (:426-460),
 * AddUECPDataFrame (:387-414), DemuxRead (:462-542) and both GetSignalStatus (:544-582).  The
 * decoder inside is an fmd_decoder; the rest is host bookkeeping like the reference's.
 * Not thread-safe by itself except write/end against demux_read (producer / consumer, like the
 * reference's source thread and demux thread). */
typedef struct fmd_receiver fmd_receiver;

#define FMD_STREAM_AUDIO 1          /* PID 1, pcm_f32le 2 ch 48 kHz (RadioReceiver.cpp:308-316) */
#define FMD_STREAM_RDS 2            /* PID 2, rds: byte-stuffed UECP frames (:326-334)          */
#define FMD_STREAM_CHANGE (-11)     /* DEMUX_SPECIALID_STREAMCHANGE                             */
#define FMD_STREAM_TIME_BASE 1000000 /* Kodi STREAM_TIME_BASE (microseconds)                    */

/* the DEMUX_PACKET fields DemuxRead fills */
typedef struct fmd_demux_packet
{
  int stream_id;       /* iStreamId                                                  */
  int size;            /* iSize, bytes                                               */
  double pts;          /* pts                                                        */
  double duration;     /* duration (audio packets only, else 0)                      */
  const uint8_t* data; /* pData: valid until the next call on this receiver          */
} fmd_demux_packet;

/* OpenLiveStream's decoder + stream state: decoder for (params), m_StreamChange = true,
 * m_PTSNext = STREAM_TIME_BASE, Reset().  tuner_freq = m_activeTunerFreq (Hz), adapter_name =
 * the RTL-SDR device name (both only appear in the status text). */
int fmd_receiver_open(const fmd_params* params, double tuner_freq, const char* adapter_name,
                      fmd_receiver** out);
void fmd_receiver_close(fmd_receiver* r);
/* WriteDataBuffer (:426-436): queues one block (copied).  _u8: cRtlSdrSource::ReadAsyncCB's input,
 * converted inside the IF kernel when the block is decoded. */
int fmd_receiver_write_iq(fmd_receiver* r, const float* iq, unsigned samples);
int fmd_receiver_write_u8(fmd_receiver* r, const uint8_t* buf, unsigned samples);
/* Any input format (FMD_IQ_*): a queued block carries its format and is decoded with it. */
int fmd_receiver_write_fmt(fmd_receiver* r, const void* buf, int format, unsigned samples);
void fmd_receiver_end(fmd_receiver* r);                 /* EndDataBuffer (:438-443)        */
size_t fmd_receiver_queued_samples(fmd_receiver* r);    /* SourceQueuedSamples (:420-424)  */
void fmd_receiver_set_stream_change(fmd_receiver* r);   /* SetStreamChange (RadioReceiver.h:83) */
/* DemuxRead (:462-542): 1 = packet filled, 0 = no packet (the reference returns nullptr: end
 * marked and queue empty), negative = error.  Order per call like the reference: stream-change
 * packet, else pending RDS bytes, else decode the next IQ block into an audio packet.  Blocks
 * while the queue is empty and the end is not marked (polling every 20 ms like :448). */
int fmd_receiver_demux_read(fmd_receiver* r, fmd_demux_packet* pkt);
/* GetSignalStatus(float&, float&, bool&) (:544-556): 1 = values valid, 0 = no decoder / stream
 * change pending (the reference returns false). */
int fmd_receiver_signal_status(fmd_receiver* r, float* interface_level_db, float* audio_level_db,
                               int* stereo);
/* GetSignalStatus(int, PVRSignalStatus&) (:558-582) */
typedef struct fmd_pvr_signal_status
{
  char adapter_name[128];
  char adapter_status[256];
  char provider_name[64]; /* m_channelName (trimmed PS name) */
  int signal;             /* SetSignal(2.5 * (interfaceLevel + 40) * 656) */
  int snr;                /* SetSNR((audioLevel + 100) * 656)             */
} fmd_pvr_signal_status;
int fmd_receiver_pvr_signal_status(fmd_receiver* r, fmd_pvr_signal_status* out);
/* the decoder inside (status getters, not to be destroyed) */
fmd_decoder* fmd_receiver_decoder(fmd_receiver* r);

/* ---- band scan: which stations a batch's captures hold ------------------------------ */
/* The reference has no channel scan (its PVR client declares SetSupportsChannelScan(false), RadioReceiver.cpp:42;
 * the tuner dialog steps 100 kHz at a time, ChannelSettings.cpp:96-147).  A scan is an averaged power spectrum of
 * every capture (Welch: nfft-point segments at a hop of nfft/2, periodic Hann window w[n] = 0.5 - 0.5 cos(2 pi n /
 * nfft)), read on the raster of the decoder's tuner steps.  fs = sample_rate_if, N = nfft, T = table_size.
 *  - Spectrum: bin i (0 .. N-1) at (i - N/2) fs / N;  P[i] = (1/K) sum over segments |sum_n w[n] x[n]
 *    e^{-j 2 pi (i - N/2) n / N}|^2 / (N sum w^2), K = the segments accumulated since the last reset (all calls).
 *    sum_i P[i] is the mean-square IQ power: a full-scale complex tone is 0 dBFS.  A call uses its S = (samples -
 *    N) / (N/2) + 1 whole segments; the samples behind the last one are not used and nothing carries over.
 *  - Slots: shift k in [-floor(T/2), -floor(T/2) + T - 1] (fmd_batch_create's tuning_shifts), centred at f(k) =
 *    -k fs / T.  Slot power = sum of P[i] over the bins within +-half_width_hz of f(k); eligible when |f(k)| +
 *    half_width_hz <= fs/2 (no wrap-around) and at least one bin lies within +-half_width_hz of f(k) (a slot
 *    narrower than a bin, 2 half_width_hz < fs / N, may hold none: it is ineligible like one at the band's edge:
 *    slot_db -inf, never a candidate, never compared with).  Floor bin = the floor(q (N-1))-th smallest P[i], q =
 *    floor_quantile; a slot's floor = floor bin x its bin count; snr_db = 10 log10(slot power / slot floor).
 *  - Candidate: an eligible slot with snr_db >= threshold_db whose power is >= that of every eligible slot within
 *    +-min_separation_hz and > that of those among them with a smaller shift.  Listed by increasing frequency.
 * Determinism: the order of every sum depends on (nfft, samples) alone and the totals (double, on the device) add
 * up in call order, so a capture gives the same bits whatever its row, the capture count or the stream.
 * Errors: FMD_ERR_ARG (with a sentence) for null arguments, a bad nfft / quantile / width, a stride shorter than
 * samples with more than one capture, a misaligned pointer (as fmd_batch_process_device[_u8]); FMD_ERR_SIZE for
 * samples < nfft; FMD_ERR_STATE for a finish with nothing accumulated.  One thread at a time per scan; the calls of
 * one scan go on one stream (or streams the caller orders).  A scan owns no stream and touches no fmd_batch. */
typedef struct fmd_scan_params
{
  double sample_rate_if;
  unsigned table_size;      /* slot raster = the cFineTuner step fs / table_size; 0 = 64 (at most 1024) */
  unsigned nfft;            /* 256..4096, power of two; 0 = 1024 */
  double half_width_hz;     /* 0 = 100e3; > 0 */
  double min_separation_hz; /* 0 = 150e3; >= 0 */
  float threshold_db;       /* 0 = 10 */
  float floor_quantile;     /* (0, 1); 0 = 0.2 */
} fmd_scan_params;
typedef struct fmd_scan_candidate
{
  int32_t shift;   /* tuner shift: fmd_batch_create's tuning_shifts / fmd_batch_retune_channels */
  float offset_hz; /* f(shift) = -shift fs / T, relative to the capture's centre */
  float power_db;  /* slot power, dBFS */
  float snr_db;    /* slot power over the slot floor */
} fmd_scan_candidate;
typedef struct fmd_scan fmd_scan;

int fmd_scan_create(const fmd_scan_params* p, unsigned n_captures, int device, fmd_scan** out);
void fmd_scan_destroy(fmd_scan* s);
/* zeroes the totals (asynchronously on stream) */
int fmd_scan_reset(fmd_scan* s, void* stream);
/* returns T; *first_shift (optional) = -floor(T/2), the shift of slot 0 */
int fmd_scan_slots(const fmd_scan* s, int32_t* first_shift);
/* Capture g starts at d_iq + 2*g*iq_capture_stride floats (bytes for _u8); byte IQ is converted like the decoder's
 * (fmd_process_stream_u8).  Asynchronous on stream. */
int fmd_scan_accumulate_device(fmd_scan* s, const float* d_iq, size_t iq_capture_stride, unsigned samples,
                               void* stream);
int fmd_scan_accumulate_device_u8(fmd_scan* s, const uint8_t* d_iq_u8, size_t iq_capture_stride, unsigned samples,
                                  void* stream);
int fmd_scan_accumulate_host(fmd_scan* s, const float* iq, size_t iq_capture_stride, unsigned samples);
/* Any input format (FMD_IQ_*), strides in IQ samples.  Signed integer IQ is converted exactly, so its scan has the
 * bits of the float scan of the converted captures (and the determinism statement above holds for it). */
int fmd_scan_accumulate_device_fmt(fmd_scan* s, const void* d_iq, int format, size_t iq_capture_stride,
                                   unsigned samples, void* stream);
int fmd_scan_accumulate_host_fmt(fmd_scan* s, const void* iq, int format, size_t iq_capture_stride,
                                 unsigned samples);
/* Outputs (each optional, NULL = not written): psd [G][N], slot_db [G][T] (-inf for an ineligible slot), floor_db
 * [G] (the floor bin), cand [G][max_cand], counts [G] (the true candidate count, also when max_cand clips the
 * list).  Does not reset: accumulation may go on, and a finish changes nothing a later finish reports.
 * Any subset of the outputs may be asked for (cand without counts, counts alone with max_cand 0, ...); the two entry
 * points give the same bits.  Capture g's list is cand[g][0 .. min(counts[g], max_cand) - 1], by increasing
 * frequency: a clipped list holds the lowest-frequency candidates.  Nothing else is written: the entries of cand
 * behind a capture's list (all of them with max_cand 0) and every byte behind an output's [G][..] extent keep what
 * the caller put there.  fmd_scan_finish_device writes asynchronously on stream.
 * A capture that held a NaN in any accumulated call: every bin of its psd is NaN (every bin of a segment depends on
 * every sample, and the totals keep it), its floor_db is NaN, slot_db is NaN for
 * every eligible slot and -inf for the others as always, and it has no candidate (counts = 0: no comparison with a NaN
 * holds) -- until fmd_scan_reset.  The call returns as usual, and the other captures keep the bits of the same scan
 * without that capture's poison. */
int fmd_scan_finish_device(fmd_scan* s, float* d_psd, float* d_slot_db, float* d_floor_db, fmd_scan_candidate* d_cand,
                           unsigned max_cand, uint32_t* d_counts, void* stream);
int fmd_scan_finish_host(fmd_scan* s, float* psd, float* slot_db, float* floor_db, fmd_scan_candidate* cand,
                         unsigned max_cand, uint32_t* counts);

/* ---- band splitter: wideband captures into decoder-rate bands --------------------------- */
/* A 10-20 MS/s capture holds the whole FM band; a batch created at that rate pays the IF stage (tuner + FIR of order
 * 8 D) per input sample and station.  The splitter is the coarse stage every SDR front end puts in front: it mixes and
 * decimates each capture ONCE into a few overlapping bands at sample_rate_in / R, ordinary FMD_IQ_F32 captures for
 * fmd_batch_process_device_fmt of a batch created at that rate (fmd_batch_set_capture_map lets any channel read any
 * band).  A band is the reference's own cFineTuner followed by cDownsampleFilter (FmDecode.cpp:45-82,
 * DownConvert.cpp:18-154) at a small integer decimation; the reference has no such stage.  Like the scan, a splitter
 * owns no stream and touches no fmd_batch; it runs asynchronously on the caller's stream.
 *
 * Geometry: G = n_captures, B = n_bands, G B output rows; row r = g B + b reads capture g and has its own tuner shift
 * shifts[r] (fmd_batch_create's tuning_shifts: the band's centre is -shift fs / T).
 * Definition.  q counts a capture's input samples since create / reset (64 bits, the same for all captures); x[q] is
 * the input sample converted as the decoder converts FMD_IQ_*; x[q] = 0 for q < 0.
 *  - Taps: c[1..K] = fmd_design_lanczos(K, cutoff)[1..K];  lut = fmd_design_tuner_lut(T, shift).
 *  - Tuner: t[q] = x[q] lut[q mod T], re = a.re*b.re - a.im*b.im, im = a.re*b.im + a.im*b.re, every operation
 *    rounded, nothing fused.
 *  - Filter: for every q that is a multiple of R, y = sum_{j = 1..K} t[q - j] c[j]: real and imaginary parts summed
 *    apart, from 0.0f, j = 1..K in order, a multiply then an add per tap, each rounded (DownConvert.cpp:117-121).
 *  - Output: the row's next sample is y * out_scale (each part).
 * A call of `samples` >= 1 delivers to every row the outputs whose q falls inside the call -- the same count for all
 * rows, known on the host when the call returns (*out_samples).  History and phase carry over calls of any size, also
 * calls shorter than K or R.  Row elements beyond the count are not written.
 * Determinism: a row's bits depend on its capture's stream, its shift and the parameters alone -- not on G, B, the
 * row's index, the tiling, the call sizes or the stream.  Non-finite and denormal input is summed as the definition
 * sums it (NaN where the definition has a NaN, bit for bit otherwise) and touches only the rows of its capture.
 * The carried state is the RAW history (the last K input samples of every capture) and q, nothing per band: so
 * fmd_split_set_shifts makes every row, from the next call submitted, bit for bit the row of a splitter that had the
 * new shifts from the start.  It does not wait for the device.
 * Errors: FMD_ERR_ARG (with a sentence naming the field) for null arguments, a parameter out of range, a format
 * outside FMD_IQ_*, a stride shorter than the call with more than one capture or row, a misaligned pointer -- all
 * before the HIP runtime is touched; FMD_ERR_DEVICE "no HIP device" without a GPU (no CPU fallback); FMD_ERR_SIZE for
 * samples of 0 or above FMD_SPLIT_MAX_SAMPLES.  One thread at a time per splitter; the calls of one splitter go on
 * one stream (or streams the caller orders).
 *
 * Real-sampled captures (fmd_split_create_real).  Wideband samplers also run in real mode: an Airspy in raw mode, a
 * direct-sampling ADC board with the FM band in its first or second Nyquist zone.  A real splitter takes such a
 * capture as it is, one element per sample (FMD_REAL_F32 / _S8 / _S16), instead of a zero Q interleaved by the host:
 *  - Definition: x[q] = (convert(v[q]), +0.0f), then everything above as it stands -- taps, tuner, filter, output,
 *    count, history, phase, fmd_split_set_shifts, reset, determinism and the non-finite rule ("touches only the rows
 *    of its capture" included).  The rows are those of a complex splitter of the same parameters fed (v, +0) pairs.
 *  - The implementation may leave out the tuner's two products with the zero part, t = (v lut.re, v lut.im).  The bits
 *    do not change: a product with +0 is a zero, and adding or subtracting a zero changes nothing but, where the
 *    other product is a zero too, that zero's sign; the zero times a tap stays a zero, and the tap sum, which starts
 *    at +0.0f and therefore never is -0, is the same with either sign added to it.  (inf and NaN: lut is finite, so
 *    the zero products are zeros there too.)
 *  - sample_rate_in is the real sample rate; a band's centre is still -shift fs / T and the output rate fs / R.  A
 *    real capture holds the station at RF f, un-inverted, at f - round(f / fs) fs in [-fs / 2, fs / 2), whatever the
 *    Nyquist zone -- and its mirror at minus that: the band filter's stopband is what removes it.
 *  - A splitter is real or complex for life: a real one takes only FMD_REAL_*, a complex one only FMD_IQ_*.  The
 *    other kind is FMD_ERR_ARG with a sentence that says which kind the splitter is (behind the null checks; the
 *    splitter stays as it was); a value that is neither is refused before anything else, as above.
 *  - Output rows are complex64 as above: FMD_IQ_F32 captures for a batch.
 * Not offered: real input anywhere but here (batch, decoder, receiver and scan refuse FMD_REAL_*; the band rows are
 * ordinary captures, and the scan takes those), unsigned 8- or 16-bit real samples, saving a splitter's state. */
#define FMD_SPLIT_MAX_SAMPLES 16777216u /* input samples per capture and call */
typedef struct fmd_split_params
{
  double sample_rate_in; /* > 0 */
  unsigned decimation;   /* R: 2..64 */
  unsigned filter_order; /* K: 2..1024; 0 = 8 R, the reference's rule (FmDecode.cpp:262) */
  double cutoff;         /* fraction of the input rate, (0, 0.5]; 0 = 0.6 / R, the reference's */
  unsigned table_size;   /* T: 1..1024; 0 = 64 */
  float out_scale;       /* any finite float; 0 = 0.5f: it undoes the tuner's factor 2, so the next decoder's
                            interface_level reads what it reads for a native capture */
} fmd_split_params;
typedef struct fmd_split fmd_split;

/* n_captures, n_bands >= 1, at most 65535 captures and 2^20 rows; shifts[n_captures * n_bands] */
int fmd_split_create(const fmd_split_params* p, unsigned n_captures, unsigned n_bands, const int* shifts, int device,
                     fmd_split** out);
/* the same parameters, ranges and defaults, for real-sampled captures (FMD_REAL_*) */
int fmd_split_create_real(const fmd_split_params* p, unsigned n_captures, unsigned n_bands, const int* shifts,
                          int device, fmd_split** out);
void fmd_split_destroy(fmd_split* s);
/* zero history, q = 0 (asynchronously on stream) */
int fmd_split_reset(fmd_split* s, void* stream);
/* new shifts for all n_rows = G B rows, from the next call submitted; returns without waiting for the device */
int fmd_split_set_shifts(fmd_split* s, const int* shifts, unsigned n_rows);
/* G B;  fs / R;  the most outputs per row a call of `samples` can deliver: ceil(samples / R) */
int fmd_split_rows(const fmd_split* s);
double fmd_split_out_rate(const fmd_split* s);
unsigned fmd_split_max_out_samples(const fmd_split* s, unsigned samples);
/* the K taps in use (c[1..K]); returns K, nothing past cap is written */
int fmd_split_get_taps(const fmd_split* s, float* out, unsigned cap);
/* Testing aids, no part of the contract above (they say how this build works inside and may change with it): the
 * input samples one workgroup's tile of outputs covers -- a whole number of R, what tests put call sizes around --
 * and how many page-locked staging versions of the tuner tables exist (one more whenever new shifts had to be
 * uploaded while every earlier upload was still in flight: fmd_split_set_shifts never waits). */
unsigned fmd_split_tile_samples(const fmd_split* s);
int fmd_split_debug_table_versions(const fmd_split* s);
/* Capture g starts g * in_capture_stride IQ samples of iq_format behind d_in (pointer and stride: multiples of two
 * IQ samples, as fmd_batch_process_device_fmt); row r starts r * out_row_stride complex64 samples behind d_out,
 * which must be 16-byte aligned, out_row_stride even (the batch needs 16-byte aligned captures) and >= the call's
 * count (fmd_split_max_out_samples always is, rounded up to even).  *out_samples (optional) = the count.
 * A real splitter: in_capture_stride and samples count real samples of iq_format (FMD_REAL_*); d_in and
 * in_capture_stride must be multiples of FOUR real samples -- 16 bytes of F32, 4 of S8, 8 of S16. */
int fmd_split_process_device(fmd_split* s, const void* d_in, int iq_format, size_t in_capture_stride, unsigned samples,
                             void* d_out, size_t out_row_stride, unsigned* out_samples, void* stream);
/* The same from and to pageable host memory, any alignment; out_row_stride any value >= the count, odd ones too
 * (rows are copied one by one through a device staging buffer).  It waits. */
int fmd_split_process_host(fmd_split* s, const void* in, int iq_format, size_t in_capture_stride, unsigned samples,
                           void* out, size_t out_row_stride, unsigned* out_samples);

/* ---- polyphase channeliser: a wideband capture's stations as channel IQ rows ------------- */
/* All stations of a wideband capture sit on one raster (100 kHz) and share one prototype low-pass: the capture is
 * filtered ONCE into its N branch sums, and every wanted station is one rotation of them -- a polyphase filter bank.
 * The rows leave at fs / D as complex64 channel IQ, what a FMD_IN_CIQ_F32 call takes in place of the IF stage: wide
 * capture -> channeliser -> FMD_IN_CIQ_F32 call, with no band rows, no capture map and no IF stage in between.  Like
 * the splitter, a channeliser owns no stream and touches no fmd_batch; it runs asynchronously on the caller's stream.
 *
 * Geometry: G = n_captures, B = n_rows_per_capture, G B output rows; row r = g B + b reads capture g and carries bin
 * shifts[r], any int, taken mod N: its centre is -shift fs / N (the convention of fmd_batch_create's tuning_shifts
 * with table_size N).  Duplicate shifts in a capture are allowed.
 * Definition (exact arithmetic).  q counts a capture's input samples since create / reset; x[q] is the input sample
 * converted as the decoder converts FMD_IQ_*; x[q] = 0 for q < 0; c[1..K] = fmd_design_lanczos(K, cutoff)[1..K], taken
 * as data.  For every q that is a multiple of D
 *     y_s[q] = out_scale * sum_{j = 1..K} x[q - j] c[j] 2 exp(+2 pi i s ((q - j) mod N) / N)
 * -- the reference's cFineTuner (table size N, shift s) followed by cDownsampleFilter, the splitter's definition with
 * T = N and R = D.  What is computed is the polyphase identity
 *     u_q[r] = sum over j with (q - j) = r (mod N) of c[j] x[q - j],   y_s[q] = 2 out_scale sum_r u_q[r] e^{2 pi i s r / N}
 * in float32, so the rows are NOT bit for bit the reference's (a filter bank cannot sum in its order); they are no less
 * accurate than the reference's own float32 arithmetic (against the definition in float64: a row's RMS error is at most
 * that of the reference's arithmetic on that row).
 * A call of `samples` >= 1 delivers to every row the outputs whose q falls inside the call -- the same count for all
 * rows, known on the host when the call returns (*out_samples).  History and phase carry over calls of any size.  Row
 * elements beyond the count are not written.
 * The carried state is the RAW history (the last K input samples of every capture) and q: fmd_chan_set_shifts makes
 * every row, from the next call submitted, bit for bit the row of a channeliser that always had those shifts, without
 * waiting for the device; fmd_chan_reset gives the rows of a new one.
 * Determinism: a row's bits depend on its capture's sample stream, its own shift and the parameters alone -- not on G,
 * B, the other rows' shifts, the row's index, the call sizes, the tiling, the stream or the entry point.
 * Non-finite input: an output whose window holds a non-finite sample is non-finite (NaN or inf, not specified) in
 * every row of that capture; every other output of that capture and every other capture keep their bits.
 * Errors, worded like the splitter's: FMD_ERR_ARG (with a sentence naming the field) for null arguments, a parameter
 * out of range, a geometry whose tile (31 D + K window samples and N branch sums of 32 output times) does not fit a
 * workgroup's LDS, a format outside FMD_IQ_* (FMD_REAL_* and FMD_IN_CIQ_* get a sentence of their own), a stride
 * shorter than the call with more than one capture or row, a misaligned pointer -- all before the HIP runtime is
 * touched; FMD_ERR_DEVICE "no HIP device" without a GPU; FMD_ERR_SIZE for samples of 0 or above FMD_CHAN_MAX_SAMPLES.
 * A refused call leaves the channeliser as it was.  One thread at a time per channeliser; its calls go on one stream
 * (or streams the caller orders).
 * Not offered by fmd_chan_create and fmd_chan_process_device / _host as such: real-sampled input (FMD_REAL_*),
 * int16 rows, saving a channeliser's state, a form for N above 256.  The first two, and N above 256 for real
 * captures, are the paragraph below.
 *
 * Real-sampled captures (fmd_chan_create_real) and rows of 16-bit integers (the _fmt entry points).  A channeliser is
 * real or complex for life.  A real one takes the same fmd_chan_params (sample_rate_in is the real sample rate; n_bins
 * 2..512, every other range and default as above) and FMD_REAL_F32 / _S8 / _S16 input, one element per sample; strides
 * and `samples` count real samples, and on the device path pointer and capture stride are multiples of FOUR samples,
 * as the real band splitter's (the host path takes any alignment).  Definition: x[q] = (convert(v[q]), +0.0f), then
 * everything above -- the output count, history and phase over calls of any size, fmd_chan_set_shifts without a wait,
 * reset, the determinism rule, the non-finite rule.  The other kind's formats are FMD_ERR_ARG with a sentence that
 * says which kind this channeliser is, and leave it as it was.
 * Contract of a real channeliser's rows.  N <= 256: a row equals, bit for bit (NaN matching NaN), the row of a complex
 * channeliser of the same parameters fed the pairs (v, +0) -- what is computed is that channeliser's chain of fmas
 * with the terms that are products of the zero imaginary parts left out, and those terms change no partial sum.  One
 * exception: an output that is a ZERO may differ in its sign (a partial sum that underflows to -0 keeps that sign only
 * until the next +0 term is added, and the two forms add different numbers of them); compare zeros with ==.
 * N in 257..512 has no complex twin: the contract is the one above -- no less accurate than the reference's float32
 * arithmetic against the definition in float64, and the determinism rule.
 * out_format belongs to the call: FMD_CIQ_F32 (complex64, what fmd_chan_process_device / _host mean; they work on both
 * kinds) or FMD_CIQ_S16: int16 re, im per sample, host byte order, fmd_f32_to_mpx16 (saturate(round_half_even(x *
 * 8192)), NaN gives 0, infinities saturate) of each part of the float the FMD_CIQ_F32 call would have stored -- exact.
 * S16 device rows: d_out 16-byte aligned, out_row_stride in complex samples, a multiple of 4 and >= the count -- the
 * rule of a FMD_IN_CIQ_S16 device call, which takes the buffer on the same stream without a copy; elements beyond the
 * count are not written.  The host path takes any stride >= the count.  Formats may change from call to call.
 * Still not offered: unsigned real samples, saving a channeliser's state, N above 256 for complex input, N above 512. */
#define FMD_CHAN_MAX_SAMPLES 16777216u /* input samples per capture and call */
typedef struct fmd_chan_params
{
  double sample_rate_in; /* > 0 */
  unsigned n_bins;       /* N: 2..256 (fmd_chan_create_real: 2..512), any integer (96, 100, 192, 200 are the real
                            ones); the raster is fs / N */
  unsigned decimation;   /* D: 2..256; the rows leave at fs / D; no relation to N is required */
  unsigned filter_order; /* K: 2..4096; 0 = 8 D, the reference's rule (FmDecode.cpp:262) */
  double cutoff;         /* fraction of the input rate, (0, 0.5]; 0 = 0.6 / D, the reference's */
  float out_scale;       /* any finite float; 0 = 1.0f: the rows carry the tuner's factor 2, as FMD_IN_CIQ_* wants */
} fmd_chan_params;
typedef struct fmd_chan fmd_chan;

/* n_captures, n_rows_per_capture >= 1, at most 65535 captures and 2^20 rows; shifts[n_captures * n_rows_per_capture] */
int fmd_chan_create(const fmd_chan_params* p, unsigned n_captures, unsigned n_rows_per_capture, const int* shifts,
                    int device, fmd_chan** out);
void fmd_chan_destroy(fmd_chan* c);
/* zero history, q = 0 (asynchronously on stream) */
int fmd_chan_reset(fmd_chan* c, void* stream);
/* new shifts for all n_rows = G B rows, from the next call submitted; returns without waiting for the device */
int fmd_chan_set_shifts(fmd_chan* c, const int* shifts, unsigned n_rows);
/* G B;  fs / D;  the most outputs per row a call of `samples` can deliver: ceil(samples / D) */
int fmd_chan_rows(const fmd_chan* c);
double fmd_chan_out_rate(const fmd_chan* c);
unsigned fmd_chan_max_out_samples(const fmd_chan* c, unsigned samples);
/* the K taps in use (c[1..K]); returns K, nothing past cap is written */
int fmd_chan_get_taps(const fmd_chan* c, float* out, unsigned cap);
/* Testing aid, no part of the contract: the input samples one workgroup's tile of outputs covers (32 D). */
unsigned fmd_chan_tile_samples(const fmd_chan* c);
/* Capture g starts g * in_capture_stride IQ samples of iq_format (FMD_IQ_F32 / _U8 / _S8 / _S16) behind d_in (pointer
 * and stride: multiples of two IQ samples, as fmd_split_process_device); row r starts r * out_row_stride complex64
 * samples behind d_out, which must be 16-byte aligned, out_row_stride even and >= the call's count
 * (fmd_chan_max_out_samples always is, rounded up to even): exactly the rows a FMD_IN_CIQ_F32 device call takes, so a
 * row buffer is handed over on the same stream without a copy.  *out_samples (optional) = the count. */
int fmd_chan_process_device(fmd_chan* c, const void* d_in, int iq_format, size_t in_capture_stride, unsigned samples,
                            void* d_out, size_t out_row_stride, unsigned* out_samples, void* stream);
/* The same from and to pageable host memory, any alignment; out_row_stride any value >= the count, odd ones too.  It
 * waits. */
int fmd_chan_process_host(fmd_chan* c, const void* in, int iq_format, size_t in_capture_stride, unsigned samples,
                          void* out, size_t out_row_stride, unsigned* out_samples);
/* A channeliser of real-sampled captures (FMD_REAL_*; the section's last paragraph): the same parameters, n_bins up to
 * 512. */
int fmd_chan_create_real(const fmd_chan_params* p, unsigned n_captures, unsigned n_rows_per_capture,
                         const int* shifts, int device, fmd_chan** out);
/* The two calls above with the rows' format, out_format = FMD_CIQ_F32 or FMD_CIQ_S16 (S16 device rows: out_row_stride
 * a multiple of 4 complex samples); either kind of channeliser, iq_format of its kind. */
int fmd_chan_process_device_fmt(fmd_chan* c, const void* d_in, int iq_format, size_t in_capture_stride,
                                unsigned samples, void* d_out, int out_format, size_t out_row_stride,
                                unsigned* out_samples, void* stream);
int fmd_chan_process_host_fmt(fmd_chan* c, const void* in, int iq_format, size_t in_capture_stride, unsigned samples,
                              void* out, int out_format, size_t out_row_stride, unsigned* out_samples);

/* ---- host-only pieces (no GPU needed) ----------------------------------------------- */
/* UECP group decoder = cRDSGroupDecoder (RDSGroupDecoder.cpp:166-1001). */
typedef struct fmd_group_decoder fmd_group_decoder;
fmd_group_decoder* fmd_group_decoder_create(const fmd_callbacks* cb, void* user, unsigned channel);
void fmd_group_decoder_destroy(fmd_group_decoder* g);
void fmd_group_decoder_reset(fmd_group_decoder* g);
void fmd_group_decoder_push(fmd_group_decoder* g, const uint16_t blocks[4]);
/* Filter design as the constructors do it on the host (float/double promotions as written):
 * cDownsampleFilter's Lanczos table (DownConvert.cpp:18-56 through the ctor :78; `order` is the
 * ctor's filter_order, order + 2 floats are written), cFirFilter::InitLPFilter's Kaiser low-pass
 * (FirFilter.cpp:44-140; returns the tap count), cIirFilter::Init (IirFilter.cpp:11-60; type
 * 0 LP, 1 HP, 2 BP, 3 BR; out = b0 b1 b2 a1 a2) and cFineTuner's table (FmDecode.cpp:45-58;
 * 2*table_size floats).  Return the element count (which may exceed cap: nothing past cap is
 * written) or -1. */
int fmd_design_lanczos(unsigned order, double cutoff, float* out, unsigned cap);
int fmd_design_lp_kaiser(float scale, float astop, float fpass, float fstop, float fs, float* out,
                         unsigned cap);
int fmd_design_biquad(int type, float f0, float q, float fs, float out[5]);
int fmd_design_tuner_lut(unsigned table_size, int freq_shift, float* out, unsigned cap);

/* cRadioReceiver::AddUECPDataFrame byte stuffing (RadioReceiver.cpp:387-414):
 * 0xFE, payload with 0xFD escapes, 0xFF.  Returns bytes written (<= cap) or -1. */
int fmd_uecp_stuff_frame(const uint8_t* frame, unsigned len, uint8_t* out, unsigned cap);

#ifdef __cplusplus
}
#endif
#endif
