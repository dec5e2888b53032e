/*
 * fmd_audio_tail.inc -- the body of the audio tail kernels (fmd_k_tail.hip.h: k_audio_tail, k_audio_tail_s16), one
 * text for every output format.  The including kernel names its output policy OUT (OutF32 / OutS16) and defines
 * FMD_TAIL_DONE_ARGS: the policy's own arguments of done(), with their leading comma, or nothing.
 * The selected forms (k_audio_tail_sel, k_audio_tail_s16_sel) also define FMD_TAIL_ROWS, the [CP] int32 table of the
 * call's selection: the output row of every channel, -1 for a channel that delivers none.  Such a lane runs the
 * recurrence, the meter and the status record like every other lane and leaves out what belongs to the output:
 * take(), store(), flush() and done() (the conversion and the clip count with them).
 * The feed forms (k_audio_tail*_feed) also define FMD_TAIL_FEED: the first of the call's rows in the feed's time-major
 * scratch ([A][CP] floats from there).  Every lane that has a channel, selected or not, stores the mono mix
 * (o.x + o.y) * 0.5f of frame i into row i: one 4-byte store a lane, 256 contiguous bytes a wave.
 * The loudness forms (fmd_k_loud.hip.h) also define FMD_TAIL_LOUD: the meter's record (LoudArgs).  Every lane,
 * selected or not, takes the float frame through the K-weighting biquads and the block sums (include/fmd.h: every
 * operation rounded on its own, in the order written there); the frame that ends a block is the same for all lanes
 * (left0, block_frames: wave-uniform), and there a lane that has a channel stores the block's 16-byte record into
 * row `slot` of the time-major ring -- 1 KB contiguous a wave -- and starts the next block from +0.
 */
  __builtin_amdgcn_s_setprio(3);
  const unsigned lane = threadIdx.x;
  // (blockDim.y channel groups per workgroup, a wave each, nothing shared: "light_pack" -- a CU that is awake for
  // one wave draws as much as one that is busy, so the light part's waves go four to a CU: MEASUREMENTS, round 5)
  const unsigned c0 = (blockIdx.x * blockDim.y + threadIdx.y) * 64 + lane;
  if (c0 - lane >= CP)
    return;
  const bool active = c0 < C;
  const unsigned c = active ? c0 : C - 1;
#ifdef FMD_TAIL_ROWS
  const int sel_row = FMD_TAIL_ROWS[c];
  const bool deliver = active && sel_row >= 0;
  const unsigned row = deliver ? (unsigned)sel_row : 0u;
  constexpr bool all_take = false;
#else
  const bool deliver = active; // one row per channel: every lane that has a channel delivers it, row = channel
  const unsigned row = c;
  constexpr bool all_take = true;
#endif
  float de_re = st.F(F_DE_RE)[c], de_im = st.F(F_DE_IM)[c];
  float w1a = st.F(F_N_W1A)[c], w2a = st.F(F_N_W2A)[c], w1b = st.F(F_N_W1B)[c], w2b = st.F(F_N_W2B)[c];
  const int stereo = st.I(I_STEREO_Q0 + (int)stereo_q)[c];
  const float one_minus_alpha = 1.0f - k.de_alpha;
  // cRadioReceiver::SamplesMeanRMS over the packet (RadioReceiver.cpp:584-598): float sums over
  // the interleaved samples L0, R0, L1, R1, ... in that order
  float vsum = 0.0f, vsumsq = 0.0f;

  auto frame = [&](float2 v) -> float2 { // v.x = stereo, v.y = mono (ProcessTwo's A, B)
    de_re = one_minus_alpha * de_re + k.de_alpha * v.x;
    const float s0 = de_re * 2.0f;
    de_im = one_minus_alpha * de_im + k.de_alpha * v.y;
    const float m0 = de_im * 2.0f;
    const float w0a = s0 - k.n_a1 * w1a - k.n_a2 * w2a;
    const float w0b = m0 - k.n_a1 * w1b - k.n_a2 * w2b;
    const float s = k.n_b0 * w0a + k.n_b1 * w1a + k.n_b2 * w2a;
    const float m = k.n_b0 * w0b + k.n_b1 * w1b + k.n_b2 * w2b;
    w2a = w1a;
    w1a = w0a;
    w2b = w1b;
    w1b = w0b;
    const float mm = m * 0.5f;
    const float2 o = stereo ? make_float2((m + s) * 0.5f, (m - s) * 0.5f) : make_float2(mm, mm);
    vsum += o.x;
    vsumsq += o.x * o.x;
    vsum += o.y;
    vsumsq += o.y * o.y;
    return o;
  };
#ifdef FMD_TAIL_LOUD
  const LoudArgs& ld = FMD_TAIL_LOUD;
  float* const __restrict__ ld_st = ld.state + c;
  const size_t ld_CP = CP;
  float ld_s[8]; // the delay words, in LoudRow order
#pragma unroll
  for (int r = 0; r < 8; r++)
    ld_s[r] = ld_st[r * ld_CP];
  float ld_zl = ld_st[LD_Z_L * ld_CP], ld_zr = ld_st[LD_Z_R * ld_CP];
  float ld_pl = ld_st[LD_PEAK_L * ld_CP], ld_pr = ld_st[LD_PEAK_R * ld_CP];
  unsigned ld_left = ld.left0, ld_slot = ld.slot0; // scalar: the same in every lane
  auto meter = [&](float2 f) {
    const float l1 = loud_biquad(f.x, ld.b0[0], ld.b1[0], ld.b2[0], ld.a1[0], ld.a2[0], ld_s[LD_S1_1L], ld_s[LD_S2_1L]);
    const float r1 = loud_biquad(f.y, ld.b0[0], ld.b1[0], ld.b2[0], ld.a1[0], ld.a2[0], ld_s[LD_S1_1R], ld_s[LD_S2_1R]);
    const float l2 = loud_biquad(l1, ld.b0[1], ld.b1[1], ld.b2[1], ld.a1[1], ld.a2[1], ld_s[LD_S1_2L], ld_s[LD_S2_2L]);
    const float r2 = loud_biquad(r1, ld.b0[1], ld.b1[1], ld.b2[1], ld.a1[1], ld.a2[1], ld_s[LD_S1_2R], ld_s[LD_S2_2R]);
    ld_zl = __fadd_rn(ld_zl, __fmul_rn(l2, l2));
    ld_zr = __fadd_rn(ld_zr, __fmul_rn(r2, r2));
    ld_pl = fmaxf(ld_pl, fabsf(f.x)); // (a NaN sample leaves the peak)
    ld_pr = fmaxf(ld_pr, fabsf(f.y));
    if (--ld_left == 0)
    { // the block ends behind this frame
      if (active)
        ld.ring[(size_t)ld_slot * ld_CP + c] = make_float4(ld_zl, ld_zr, ld_pl, ld_pr);
      ld_zl = ld_zr = ld_pl = ld_pr = 0.0f;
      ld_left = ld.block_frames;
      ld_slot = ld_slot + 1 == ld.ring_blocks ? 0u : ld_slot + 1;
    }
  };
#endif
  typename OUT::frame_t* __restrict__ o = reinterpret_cast<typename OUT::frame_t*>(audio + (size_t)row * audio_stride);
  typename OUT::State os;

  unsigned i0 = 0;
  // full tiles: the loads of the next tile are in flight while this one goes through the recurrence
  // out of registers (past the last full tile: clamped rows nobody uses)
  float2 vnext[AT_STEPS];
#pragma unroll
  for (unsigned u = 0; u < AT_STEPS; u++)
    vnext[u] = lp[(size_t)min(u, A - 1) * CP + c];
  for (; i0 + AT_STEPS <= A; i0 += AT_STEPS)
  {
    float2 vin[AT_STEPS];
#pragma unroll
    for (unsigned u = 0; u < AT_STEPS; u++)
      vin[u] = vnext[u];
#pragma unroll
    for (unsigned u = 0; u < AT_STEPS; u++)
      vnext[u] = lp[(size_t)min(i0 + AT_STEPS + u, A - 1) * CP + c];
#pragma unroll
    for (unsigned u = 0; u < AT_STEPS; u++)
    {
      const float2 f = frame(vin[u]);
#ifdef FMD_TAIL_LOUD
      meter(f);
#endif
#ifdef FMD_TAIL_FEED
      if (active)
        FMD_TAIL_FEED[(size_t)(i0 + u) * CP + c] = (f.x + f.y) * 0.5f;
#endif
      if (all_take || deliver)
        OUT::take(os, u, f);
      if (deliver)
        OUT::store(o, os, i0, u, f);
    }
  }
  if (i0 < A)
  {
    const unsigned cnt = A - i0;
#pragma unroll
    for (unsigned u = 0; u < AT_STEPS; u++) // the ragged last tile is already in vnext
      if (u < cnt)
      {
        const float2 f = frame(vnext[u]);
#ifdef FMD_TAIL_LOUD
        meter(f);
#endif
#ifdef FMD_TAIL_FEED
        if (active)
          FMD_TAIL_FEED[(size_t)(i0 + u) * CP + c] = (f.x + f.y) * 0.5f;
#endif
        if (all_take || deliver)
          OUT::take(os, u, f);
        if (deliver)
          OUT::store(o, os, i0, u, f);
      }
    OUT::flush(o, os, i0, cnt, deliver);
  }
  if (active)
  {
#ifdef FMD_TAIL_LOUD
#pragma unroll
    for (int r = 0; r < 8; r++)
      ld_st[r * ld_CP] = ld_s[r];
    ld_st[LD_Z_L * ld_CP] = ld_zl;
    ld_st[LD_Z_R * ld_CP] = ld_zr;
    ld_st[LD_PEAK_L * ld_CP] = ld_pl;
    ld_st[LD_PEAK_R * ld_CP] = ld_pr;
#endif
    st.F(F_DE_RE)[c] = de_re;
    st.F(F_DE_IM)[c] = de_im;
    st.F(F_N_W1A)[c] = w1a;
    st.F(F_N_W2A)[c] = w2a;
    st.F(F_N_W1B)[c] = w1b;
    st.F(F_N_W2B)[c] = w2b;
    // mean = vsum / n, rms = sqrt(vsumsq / n) in float (n = floats in the packet), then
    // m_AudioLevel = 0.95 * m_AudioLevel + 0.05 * audio_rms in double (RadioReceiver.cpp:526-528)
    const float n = (float)(2u * A);
    const float rms = sqrtf(vsumsq / n);
    const float mean = vsum / n;
    const float level = (float)(0.95 * (double)st.F(F_AUDIO_LEVEL)[c] + 0.05 * (double)rms);
    st.F(F_AUDIO_MEAN)[c] = mean;
    st.F(F_AUDIO_RMS)[c] = rms;
    st.F(F_AUDIO_LEVEL)[c] = level;
    /* The call is complete for this channel: its status record (see HostStatusWord).  The level
     * meters are the state arrays as they stand now; the stereo flag is this call's own copy.  With
     * overlapped calls (concurrency 2) the next call's IF / baseband meters may already be in -- the
     * reference's status thread reads its decoder mid-call too (RadioReceiver.cpp:544-572 against
     * :524, no common lock). */
    unsigned* __restrict__ h = st.ds + c;
    const size_t CPs = st.CP;
    h[HS_IF_LEVEL * CPs] = __float_as_uint(st.F(F_IF_LEVEL)[c]);
    h[HS_BB_MEAN * CPs] = __float_as_uint(st.F(F_BB_MEAN)[c]);
    h[HS_BB_LEVEL * CPs] = __float_as_uint(st.F(F_BB_LEVEL)[c]);
    h[HS_P_LEVEL * CPs] = __float_as_uint(st.F(F_P_LEVEL)[c]);
    h[HS_STEREO * CPs] = (unsigned)stereo;
    h[HS_AUDIO_MEAN * CPs] = __float_as_uint(mean);
    h[HS_AUDIO_RMS * CPs] = __float_as_uint(rms);
    h[HS_AUDIO_LEVEL * CPs] = __float_as_uint(level);
    if (all_take || deliver)
      OUT::done(os, c FMD_TAIL_DONE_ARGS);
  }
