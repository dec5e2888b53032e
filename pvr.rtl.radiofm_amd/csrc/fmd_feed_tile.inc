/*
 * fmd_feed_tile.inc -- the body of the feed writers (fmd_k_feed.hip.h: k_feed_out, k_feed_out_sel), one text for
 * both: a tile of 64 rows x FEED_T outputs of the decimating filter, through the LDS image described there.  The
 * including kernel names its store policy Fmt and defines which rows the tile holds, from row0 = 64 blockIdx.x:
 * FMD_FEED_SRC(c) the channel tile row c reads, FMD_FEED_SKIPPED(c) whether tile row c is not stored,
 * FMD_FEED_DST(c) the output row it is stored to.
 */
  __shared__ __attribute__((aligned(16))) float tile[64 * FEED_T];
  __shared__ float hs[FEED_TAPS_MAX + 1];
  const unsigned l = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned row0 = blockIdx.x * 64u, t0 = blockIdx.y * FEED_T;
  if (threadIdx.x < T)
    hs[threadIdx.x] = taps[threadIdx.x];
  __syncthreads();
  {
    const unsigned c = (l & 48u) + 2u * (l & 7u) + ((l >> 3) & 1u);
    // the lane's channel in row (T - 1) + p0 of the scratch: x[n D] of the call's first output n
    const float* src = x + size_t(T - 1u + p0) * CP + size_t(FMD_FEED_SRC(c));
    float4 v[4];
#pragma unroll
    for (unsigned jj = 0; jj < 4; jj++)
    {
      const unsigned j = t0 + 4u * (w + 4u * jj);
      // (outputs at or behind n: the call's last one is computed again, none of them is stored)
      const float* p[4];
      float acc[4];
#pragma unroll
      for (unsigned e = 0; e < 4; e++)
      {
        p[e] = src + size_t(min(j + e, n - 1u)) * D * CP;
        acc[e] = 0.0f;
      }
      if (j < n) // (the wave's: j is wave-uniform)
      {
#pragma unroll 4
        for (unsigned k = 0; k < T; k++)
        { // acc = acc + h[k] * x[n D - k], k ascending, the product and the sum rounded one after the other
          const float h = hs[k];
#pragma unroll
          for (unsigned e = 0; e < 4; e++)
          {
            acc[e] = __fadd_rn(acc[e], __fmul_rn(h, *p[e]));
            p[e] -= CP;
          }
        }
      }
      v[jj] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
#pragma unroll
    for (unsigned jj = 0; jj < 4; jj++)
      *reinterpret_cast<float4*>(&tile[c * FEED_T + 4u * ((w + 4u * jj + (c >> 1)) & 15u)]) = v[jj];
  }
  __syncthreads();
  constexpr unsigned PER = Fmt::PER;       // samples a lane stores at a time
  constexpr unsigned LPR = FEED_T / PER;   // lanes per channel row of the tile: 16 / 8
  constexpr unsigned CPI = 64u / LPR;      // channels per wave and read: 4 / 8
  constexpr unsigned NI = 16u / CPI;       // groups of PER samples per lane: 4 / 2
  const unsigned g = l % LPR;              // the lane's group of PER samples in its channels' rows
  const unsigned t = t0 + PER * g;
  float y[NI][PER];
#pragma unroll
  for (unsigned i = 0; i < NI; i++)
  {
    const unsigned c = 16u * w + CPI * i + l / LPR;
#pragma unroll
    for (unsigned s = 0; s < PER / 4u; s++)
    {
      const float4 f =
          *reinterpret_cast<const float4*>(&tile[c * FEED_T + 4u * (((PER / 4u) * g + s + (c >> 1)) & 15u)]);
      y[i][4 * s] = f.x;
      y[i][4 * s + 1] = f.y;
      y[i][4 * s + 2] = f.z;
      y[i][4 * s + 3] = f.w;
    }
  }
  const bool whole = t0 + FEED_T <= n; // (the workgroup's: every tile but the call's last one)
#pragma unroll
  for (unsigned i = 0; i < NI; i++)
  {
    const unsigned c = 16u * w + CPI * i + l / LPR;
    if (FMD_FEED_SKIPPED(c))
      continue;
    typename Fmt::elem_t* o = out + size_t(FMD_FEED_DST(c)) * stride + t;
    if constexpr (PER == 4)
    {
      if (whole)
        *reinterpret_cast<float4*>(o) = make_float4(y[i][0], y[i][1], y[i][2], y[i][3]);
      else
      { // (volatile: the compiler otherwise folds these stores into the 16-byte one and splits that in 12 + 4)
        volatile float* ov = o;
#pragma unroll
        for (unsigned e = 0; e < 4; e++)
          if (t + e < n)
            ov[e] = y[i][e];
      }
    }
    else
    {
      unsigned h[8];
#pragma unroll
      for (unsigned e = 0; e < 8; e++)
        h[e] = (unsigned)fmd_f32_to_s16(y[i][e]) & 0xffffu;
      if (whole)
        *reinterpret_cast<uint4*>(o) =
            make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
      else
      {
        volatile int16_t* ov = o;
#pragma unroll
        for (unsigned e = 0; e < 8; e++)
          if (t + e < n)
            ov[e] = (int16_t)h[e];
      }
    }
  }
