/*
 * fmd_mpx_tile.inc -- the body of the multiplex writers (fmd_k_mpx.hip.h: k_mpx_out, k_mpx_out_sel), one text for
 * both: a tile of 64 rows x MPX_T time steps through the LDS image described there.  The including kernel names its
 * store policy Fmt and defines which rows the tile holds, from row0 = 64 blockIdx.x: FMD_MPX_SRC(c) the channel tile
 * row c reads, FMD_MPX_SKIPPED(c) whether tile row c is not stored, FMD_MPX_DST(c) the output row it is stored to.
 */
  __shared__ __attribute__((aligned(16))) float tile[64 * MPX_T];
  const unsigned l = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned row0 = blockIdx.x * 64u, t0 = blockIdx.y * MPX_T;
  {
    const unsigned c = (l & 48u) + 2u * (l & 7u) + ((l >> 3) & 1u);
    const float* src = in + 2u * size_t(FMD_MPX_SRC(c));
    float4 v[4];
#pragma unroll
    for (unsigned jj = 0; jj < 4; jj++)
    {
      const unsigned t = t0 + 4u * (w + 4u * jj);
      float x[4];
#pragma unroll
      for (unsigned e = 0; e < 4; e++)
        x[e] = (t + e < M) ? src[2u * size_t(t + e) * CP] : 0.0f;
      v[jj] = make_float4(x[0], x[1], x[2], x[3]);
    }
#pragma unroll
    for (unsigned jj = 0; jj < 4; jj++)
      *reinterpret_cast<float4*>(&tile[c * MPX_T + 4u * ((w + 4u * jj + (c >> 1)) & 15u)]) = v[jj];
  }
  __syncthreads();
  constexpr unsigned PER = Fmt::PER;       // samples a lane stores at a time
  constexpr unsigned LPR = MPX_T / PER;    // lanes per channel row of the tile: 16 / 8
  constexpr unsigned CPI = 64u / LPR;      // channels per wave and read: 4 / 8
  constexpr unsigned NI = 16u / CPI;       // groups of PER samples per lane: 4 / 2
  const unsigned g = l % LPR;              // the lane's group of PER samples in its channels' rows
  const unsigned t = t0 + PER * g;
  float x[NI][PER];
#pragma unroll
  for (unsigned i = 0; i < NI; i++)
  {
    const unsigned c = 16u * w + CPI * i + l / LPR;
#pragma unroll
    for (unsigned s = 0; s < PER / 4u; s++)
    {
      const float4 f =
          *reinterpret_cast<const float4*>(&tile[c * MPX_T + 4u * (((PER / 4u) * g + s + (c >> 1)) & 15u)]);
      x[i][4 * s] = f.x;
      x[i][4 * s + 1] = f.y;
      x[i][4 * s + 2] = f.z;
      x[i][4 * s + 3] = f.w;
    }
  }
  const bool whole = t0 + MPX_T <= M; // (the workgroup's: every tile but the call's last one)
#pragma unroll
  for (unsigned i = 0; i < NI; i++)
  {
    const unsigned c = 16u * w + CPI * i + l / LPR;
    if (FMD_MPX_SKIPPED(c))
      continue;
    typename Fmt::elem_t* o = out + size_t(FMD_MPX_DST(c)) * stride + t;
    if constexpr (PER == 4)
    {
      if (whole)
        *reinterpret_cast<float4*>(o) = make_float4(x[i][0], x[i][1], x[i][2], x[i][3]);
      else
      { // (volatile: the compiler otherwise folds these stores into the 16-byte one and splits that in 12 + 4)
        volatile float* ov = o;
#pragma unroll
        for (unsigned e = 0; e < 4; e++)
          if (t + e < M)
            ov[e] = x[i][e];
      }
    }
    else
    {
      unsigned h[8];
#pragma unroll
      for (unsigned e = 0; e < 8; e++)
        h[e] = (unsigned)fmd_f32_to_mpx16(x[i][e]) & 0xffffu;
      if (whole)
        *reinterpret_cast<uint4*>(o) =
            make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
      else
      {
        volatile int16_t* ov = o;
#pragma unroll
        for (unsigned e = 0; e < 8; e++)
          if (t + e < M)
            ov[e] = (int16_t)h[e];
      }
    }
  }
