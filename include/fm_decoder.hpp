/*
 * fm_decoder.hpp -- the reference's cFmDecoder class surface on top of the C ABI (fmd.h).
 *
 * A caller written against src/FmDecode.h:91-225 of AlwinEsch/pvr.rtl.radiofm (in practice
 * cRadioReceiver, src/RadioReceiver.cpp:296-300, :349, :373, :524-525, :551-553, :565-572)
 * compiles against this header unchanged: same class name, constructor signature, method names,
 * argument meaning and return values.  The three upward calls the RDS group decoder makes into
 * cRadioReceiver (AddUECPDataFrame / SetChannelName / IsSettingActive, RadioReceiver.h:77,80,115)
 * are forwarded through fmd_callbacks to the `proc` object handed to the constructor.
 *
 * Header-only; link with libfmd_hip.so.  Errors of the GPU library (the reference has no error
 * path) are reported by throwing std::runtime_error from the constructor and by returning 0
 * audio samples from ProcessStream.
 */
#pragma once

#include <complex>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "fmd.h"

typedef std::complex<float> ComplexType; // Definitions.h:44
typedef float RealType;                  // Definitions.h:45

#ifndef DEFAULT_BANDWIDTH_PCM
#define DEFAULT_BANDWIDTH_PCM 15000.0 // FmDecode.h:24
#endif

/* Receiver: any class with
 *   bool AddUECPDataFrame(uint8_t* frame, unsigned int len);
 *   bool SetChannelName(std::string name);
 *   bool IsSettingActive();
 * i.e. cRadioReceiver's members.  The class cFmDecoder at the bottom binds it to the class named
 * cRadioReceiver, like FmDecode.h does (:27). */
template <class Receiver>
class cFmDecoderT
{
public:
  cFmDecoderT(Receiver* proc,
              double sample_rate_if,
              double tuning_offset,
              double sample_rate_pcm,
              double bandwidth_pcm = DEFAULT_BANDWIDTH_PCM,
              unsigned int downsample = 1,
              bool USver = false)
    : m_proc(proc)
  {
    fmd_params p{};
    p.sample_rate_if = sample_rate_if;
    p.tuning_offset = tuning_offset;
    p.sample_rate_pcm = sample_rate_pcm;
    p.bandwidth_pcm = bandwidth_pcm;
    p.downsample = downsample;
    p.us_version = USver ? 1 : 0;
    fmd_callbacks cb{};
    cb.add_uecp_frame = &cFmDecoderT::OnFrame;
    cb.set_channel_name = &cFmDecoderT::OnName;
    cb.is_setting_active = &cFmDecoderT::OnActive;
    if (fmd_create(&p, &cb, this, &m_dec) != FMD_OK)
      throw std::runtime_error(std::string("cFmDecoder: ") + fmd_last_error());
  }

  virtual ~cFmDecoderT() { fmd_destroy(m_dec); }

  cFmDecoderT(const cFmDecoderT&) = delete;
  cFmDecoderT& operator=(const cFmDecoderT&) = delete;

  void Reset() { fmd_reset(m_dec); }

  /* FmDecode.h:135 -- returns the number of floats written to `audio` (2 per frame) */
  unsigned int ProcessStream(const ComplexType* samples_in, unsigned int samples, float* audio)
  {
    const int n = fmd_process_stream(m_dec, reinterpret_cast<const float*>(samples_in), samples, audio);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }

  /* Not in the reference: cRtlSdrSource::ReadAsyncCB's conversion (RTL_SDR_Source.cpp:206-211)
   * and ProcessStream in one call -- buf = 2 * samples bytes as librtlsdr delivers them. */
  unsigned int ProcessStreamU8(const uint8_t* buf, unsigned int samples, float* audio)
  {
    const int n = fmd_process_stream_u8(m_dec, buf, samples, audio);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }

  /* Not in the reference: signed integer IQ as HackRF (8 bits) and Airspy, SDRplay, USRP sc16, .cs16 files (16
   * bits) deliver it -- buf = 2 * samples values I, Q, I, Q, ..., full scale = [-1, 1) (v * 2^-7, v * 2^-15). */
  unsigned int ProcessStreamS8(const int8_t* buf, unsigned int samples, float* audio)
  {
    const int n = fmd_process_stream_fmt(m_dec, buf, FMD_IQ_S8, samples, audio);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }
  unsigned int ProcessStreamS16(const int16_t* buf, unsigned int samples, float* audio)
  {
    const int n = fmd_process_stream_fmt(m_dec, buf, FMD_IQ_S16, samples, audio);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }

  /* Not in the reference: ProcessStream with the audio as interleaved signed 16-bit PCM, L, R, L, R, ... --
   * saturate(round_half_even(x * 32768)) of the float sample ProcessStream writes (FMD_PCM_S16); returns the number
   * of int16 samples written (2 per frame).  Calls of the two may follow each other freely. */
  unsigned int ProcessStreamToPcm16(const ComplexType* samples_in, unsigned int samples, int16_t* audio)
  {
    const int n = fmd_process_stream_pcm(m_dec, samples_in, FMD_IQ_F32, samples, audio, FMD_PCM_S16);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }

  bool StereoDetected() const { return Status().stereo_detected != 0; }
  RealType GetTuningOffset() const { return Status().tuning_offset; }
  RealType GetInterfaceLevel() const { return Status().interface_level; }
  RealType GetBasebandLevel() const { return Status().baseband_level; }
  RealType GetPilotLevel() const { return Status().pilot_level; }

  /* Not in the reference: the decoder's whole state as an opaque blob and back (fmd_save_state / fmd_load_state).
   * SaveState returns the bytes written (0 on an error; blob == nullptr or cap too small: the bytes needed are in
   * *needed where given); a decoder constructed with the same arguments continues the stream bit for bit after
   * LoadState (true on success; fmd_last_error() says why not). */
  size_t SaveState(void* blob, size_t cap, size_t* needed = nullptr)
  {
    size_t n = fmd_batch_state_size(fmd_decoder_batch(m_dec), 1);
    if (needed)
      *needed = n;
    if (!blob || cap < n)
      return 0;
    return fmd_save_state(m_dec, blob, cap, &n) == FMD_OK ? n : 0;
  }
  bool LoadState(const void* blob, size_t size) { return fmd_load_state(m_dec, blob, size) == FMD_OK; }

  /* Not in the reference: ProcessStream with the demodulated multiplex beside the audio -- the FM PLL's output at
   * the baseband rate (m_BufferBaseband, FmDecode.cpp:433; a deviation of f Hz reads f / 30 000), *mpx_samples floats
   * into `mpx`, a caller buffer of `samples` floats (FMD_MPX_F32).  The audio is ProcessStream's. */
  unsigned int ProcessStreamWithMpx(const ComplexType* samples_in, unsigned int samples, float* audio, float* mpx,
                                    unsigned int* mpx_samples)
  {
    const int n = fmd_process_stream_mpx(m_dec, samples_in, FMD_IQ_F32, samples, audio, FMD_PCM_F32, mpx, FMD_MPX_F32,
                                         mpx_samples);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }

  /* Not in the reference: a mono feed at sample_rate_pcm / divisor beside the audio (fmd.h, FMD_FEED_*), what a
   * speech or fingerprinting model takes.  SetFeed(2 or 3) turns it on and zeroes its history, SetFeed(0) turns it
   * off; ProcessStreamWithFeed writes *feed_samples 16-bit samples into `feed`, a caller buffer of
   * samples / divisor + 1 elements at least.  The audio is ProcessStream's. */
  bool SetFeed(int divisor) { return fmd_batch_set_feed(fmd_decoder_batch(m_dec), divisor) == FMD_OK; }
  unsigned int ProcessStreamWithFeed(const ComplexType* samples_in, unsigned int samples, float* audio,
                                     int16_t* feed, unsigned int* feed_samples)
  {
    const int n = fmd_process_stream_feed(m_dec, samples_in, FMD_IQ_F32, samples, audio, FMD_PCM_F32, feed,
                                          FMD_FEED_S16, feed_samples);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }

  /* Not in the reference: the station's complex baseband behind tuner and IF filter beside the audio (fmd.h,
   * FMD_CIQ_*; m_BufferIF, the samples the FM PLL demodulates), at sample_rate_if / downsample.  Writes *ciq_samples
   * complex samples into `ciq`, a caller buffer of `samples` elements at least.  The audio is ProcessStream's. */
  unsigned int ProcessStreamWithChannelIq(const ComplexType* samples_in, unsigned int samples, float* audio,
                                          ComplexType* ciq, unsigned int* ciq_samples)
  {
    fmd_call c{};
    c.size = sizeof(fmd_call);
    c.iq = samples_in;
    c.iq_format = FMD_IQ_F32;
    c.samples = samples;
    c.audio.p = audio;
    c.audio.format = FMD_PCM_F32;
    c.ciq.p = ciq;
    c.ciq.format = FMD_CIQ_F32;
    c.ciq.count = ciq_samples;
    const int n = fmd_process_stream_call(m_dec, &c);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }

  /* Not in the reference: the way back in -- one call from the station's complex baseband behind tuner and IF filter
   * (fmd.h, FMD_IN_CIQ_*), `m` complex samples (re, im floats) at sample_rate_if / downsample: what
   * ProcessStreamWithChannelIq delivered, from an archive, or a channeliser's of the caller's own.  The IF stage does
   * not run and keeps its state; everything behind it takes the samples as its output.  The audio as ProcessStream
   * writes it; returns the floats written.  ProcessChannelIqToPcm16 / ProcessChannelIqWithMpx: the record form with
   * the audio as int16 (FMD_PCM_S16) / with the multiplex beside it (`mpx`: a buffer of m floats). */
  unsigned int ProcessChannelIq(const float* ciq, unsigned int m, float* audio)
  {
    return ChannelIqCall(ciq, m, audio, FMD_PCM_F32, nullptr, nullptr);
  }
  unsigned int ProcessChannelIqToPcm16(const float* ciq, unsigned int m, int16_t* audio)
  {
    return ChannelIqCall(ciq, m, audio, FMD_PCM_S16, nullptr, nullptr);
  }
  unsigned int ProcessChannelIqWithMpx(const float* ciq, unsigned int m, float* audio, float* mpx,
                                       unsigned int* mpx_samples)
  {
    return ChannelIqCall(ciq, m, audio, FMD_PCM_F32, mpx, mpx_samples);
  }

  /* Not in the reference: what its block synchroniser computes and drops (fmd.h, "Every RDS block decision").
   * SetRdsBlocks: the observation of every ProcessStream from now on (FMD_RDS_BLOCKS_*); CollectRdsBlocks: the block
   * records queued so far, in order, into `out` (returns their number; *lost: records that did not fit);
   * GetRdsQuality: the reception counters since the decoder was made (no Reset clears them). */
  bool SetRdsBlocks(int mode, unsigned int queue_records = 0)
  {
    return fmd_batch_set_rds_blocks(fmd_decoder_batch(m_dec), mode, queue_records) == FMD_OK;
  }
  unsigned int CollectRdsBlocks(fmd_rds_block* out, unsigned int cap, unsigned int* lost = nullptr)
  {
    const int n = fmd_batch_collect_rds_blocks(fmd_decoder_batch(m_dec), out, cap, 0, nullptr, lost);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }
  bool GetRdsQuality(fmd_rds_quality* out)
  {
    return fmd_batch_read_rds_quality(fmd_decoder_batch(m_dec), 0, 1, out) == FMD_OK;
  }

  /* Not in the reference: ITU-R BS.1770 loudness blocks of the audio (fmd.h, "loudness blocks").  SetLoudness: the
   * meter of every ProcessStream from now on (block_frames 0: 100 ms, ring_blocks 0: 64; fixed the first time it is
   * turned on); CollectLoudness: the blocks completed and not yet collected, in order, into `out` (returns their
   * number; *first_block: the index of the first; *lost: blocks the ring had overwritten).  fmd_loudness_window /
   * fmd_loudness_integrated turn them into LUFS. */
  bool SetLoudness(bool on, unsigned int block_frames = 0, unsigned int ring_blocks = 0)
  {
    return fmd_batch_set_loudness(fmd_decoder_batch(m_dec), on ? FMD_LOUDNESS_ON : FMD_LOUDNESS_OFF, block_frames,
                                  ring_blocks) == FMD_OK;
  }
  unsigned int CollectLoudness(fmd_loud_block* out, unsigned int cap_blocks, uint64_t* first_block = nullptr,
                               unsigned int* lost = nullptr)
  {
    const int n =
        fmd_batch_collect_loudness(fmd_decoder_batch(m_dec), out, cap_blocks, 0, 1, 0, nullptr, first_block, lost);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }

private:
  unsigned int ChannelIqCall(const float* ciq, unsigned int m, void* audio, int pcm_format, float* mpx,
                             unsigned int* mpx_samples)
  {
    fmd_call c{};
    c.size = sizeof(fmd_call);
    c.iq = ciq;
    c.iq_format = FMD_IN_CIQ_F32;
    c.samples = m;
    c.audio.p = audio;
    c.audio.format = pcm_format;
    c.mpx.p = mpx;
    c.mpx.format = FMD_MPX_F32;
    c.mpx.count = mpx_samples;
    const int n = fmd_process_stream_call(m_dec, &c);
    return n > 0 ? static_cast<unsigned int>(n) : 0u;
  }
  fmd_status Status() const
  {
    fmd_status st{};
    fmd_get_status(m_dec, &st);
    return st;
  }
  static int OnFrame(void* user, unsigned, const uint8_t* frame, unsigned len)
  {
    auto* self = static_cast<cFmDecoderT*>(user);
    return self->m_proc && self->m_proc->AddUECPDataFrame(const_cast<uint8_t*>(frame), len) ? 1 : 0;
  }
  static int OnName(void* user, unsigned, const char name[9])
  {
    auto* self = static_cast<cFmDecoderT*>(user);
    return self->m_proc && self->m_proc->SetChannelName(std::string(name, 8)) ? 1 : 0;
  }
  static int OnActive(void* user, unsigned)
  {
    auto* self = static_cast<cFmDecoderT*>(user);
    return self->m_proc && self->m_proc->IsSettingActive() ? 1 : 0;
  }

  Receiver* const m_proc;
  fmd_decoder* m_dec = nullptr;
};

#ifndef FMD_NO_CFMDECODER_ALIAS
/* The reference's name, as a real class: RadioReceiver.h:23 forward-declares `class cFmDecoder;`
 * and keeps a `cFmDecoder*` member (:124) before any decoder header is seen, so the name must be
 * a class (a typedef would conflict with that declaration).  cRadioReceiver may still be
 * incomplete here (FmDecode.h:27 only forward-declares it too): the base template's members that
 * call into it are instantiated where they are used -- `new cFmDecoder(this, ...)` at
 * RadioReceiver.cpp:296-300, where the class is complete. */
class cRadioReceiver; // FmDecode.h:27
class cFmDecoder : public cFmDecoderT<cRadioReceiver>
{
public:
  using cFmDecoderT<cRadioReceiver>::cFmDecoderT;
};
#endif
