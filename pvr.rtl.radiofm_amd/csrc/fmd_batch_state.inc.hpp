/*
 * fmd_batch_state.inc.hpp -- a running batch's state out of the device and back: fmd_batch_save_state /
 * fmd_batch_load_state (the whole batch), fmd_batch_export_channels / fmd_batch_import_channels (single channels,
 * from one batch into another) and the single decoder's pair (include/fmd.h).  Included by
 * fmd_batch.hip behind the batch's C ABI (one translation unit: it uses that file's fmd_batch struct and helpers).
 *
 * The blob, all sections 8-byte aligned:
 *   StateHeader | kOscH oscillator entries | n host records | n-channel payload | the twin's 1-channel payload
 * A payload holds every region of the batch's StateTable packed [row][n] (fmd_k_state.hip.h); a host record holds
 * what the host keeps per channel (shift, capture, the status snapshot, the group decoder).
 */
namespace
{

constexpr uint64_t kStateMagic = 0x31304554415453dfull; // reads differently on a host of the other byte order
constexpr uint32_t kStateLayout = 1;
enum StateFlag : uint32_t
{
  SF_WHOLE = 1,    // a whole batch (fmd_batch_save_state): clock, capture map and call index are the batch's to take
  SF_TWIN = 2,     // retuning was enabled: the silent twin's payload follows
  SF_ORIGINS = 4,  // some ring origin is not the batch's phase (origins_live)
  SF_OSC = 8,      // the batch kept the oscillator sequence: its last entries and (osc_re, osc_im) are valid
  SF_MAP = 16      // a capture map (else the cpc rule)
};
/* Skip indices of fmd_batch_debug_state_skip behind the restart's regions */
constexpr int kSkipStatus = kRestartRegionCount, kSkipGdec = kRestartRegionCount + 1,
              kSkipMeter = kRestartRegionCount + 2, kSkipCount = kRestartRegionCount + 3;

struct StateClock
{
  uint32_t if_pos, lut_idx;
  float rs_pos;
  uint32_t rds_lpf_g, mf_g, alpf_g;
  int32_t hist_sel;
  uint32_t call_index;
  float osc_re, osc_im;
  uint32_t lastM, lastA, lastR, pad;
};

struct StateHeader
{
  uint64_t magic;
  uint32_t layout, header_bytes;
  char version[32];
  uint64_t fingerprint;
  uint32_t n_channels, flags;
  StateClock clock;
  uint32_t cpc, n_cap;
  uint64_t total_bytes;
  uint64_t checksum; // FNV-1a 64 over the whole blob with this field zero
};
static_assert(sizeof(StateHeader) % 8 == 0, "sections stay 8-byte aligned");

struct StateHostRec
{
  int32_t shift;
  uint32_t capture;
  uint32_t has_gdec, pad;
  uint32_t status[fmd::HS_WORDS + (fmd::HS_WORDS & 1)]; // the getters' snapshot, tags included
};
static_assert(sizeof(StateHostRec) % 8 == 0, "sections stay 8-byte aligned");

uint64_t fnv1a(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ull)
{
  const unsigned char* c = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; i++)
    h = (h ^ c[i]) * 0x100000001b3ull;
  return h;
}

size_t gdec_bytes()
{
  static const size_t n = [] {
    fmd::GroupDecoder g(nullptr, nullptr, 0);
    size_t s = 0;
    g.each_field([&](void*, size_t k) { s += k; });
    return (s + 7) & ~size_t(7);
  }();
  return n;
}

size_t host_rec_bytes()
{
  return sizeof(StateHostRec) + gdec_bytes();
}

constexpr size_t kOscBytes = size_t(fmd_batch::kOscH) * sizeof(fmd::HbOsc);

/* state_tab of a batch with buffers of its own: its carried regions (carried_regions, what a restart copies) with the
 * audio meter's rows of the float state as a group of their own, then the status record and the clip counter */
int ensure_state_table(fmd_batch* x)
{
  if (x->state_tab.n)
    return FMD_OK;
  fmd::StateTable t{};
  size_t off = 0;
  bool full = false;
  auto put = [&](int group, void* base, unsigned rows, unsigned esz, size_t row, size_t ch) {
    if (rows == 0)
      return;
    if (t.n >= fmd::kStateMaxRegions)
    {
      full = true;
      return;
    }
    x->state_group[t.n] = group;
    t.r[t.n++] = fmd::StateRegion{base, rows, esz, row, ch, off};
    off += (size_t(rows) * esz + 7) & ~size_t(7);
  };
  const size_t CP = x->CP;
  static_assert(fmd::F_AUDIO_MEAN + 3 == fmd::F_SLOTS, "the audio meter's slots are the last three");
  for (const CarriedRegion& r : carried_regions(x))
    if (r.base == x->fstate.p)
    { // the audio meter belongs to the output: loads and imports may leave it out with the clip counter
      put(r.group, r.base, fmd::F_AUDIO_MEAN, r.esz, r.row, r.ch);
      put(kSkipMeter, x->st.F(fmd::F_AUDIO_MEAN), r.rows - fmd::F_AUDIO_MEAN, r.esz, r.row, r.ch);
    }
    else
      put(r.group, r.base, r.rows, r.esz, r.row, r.ch);
  put(kSkipStatus, x->d_status.p, fmd::HS_WORDS, 4, CP, 1);
  put(kSkipMeter, x->pcm_clip.p, 1, 8, CP, 1);
  if (full)
    return fail(FMD_ERR_ARG, "this geometry has more carried regions than a state table takes");
  x->state_tab = t;
  x->state_bytes = off;
  for (auto& e : x->imp_ev)
    HIPCHK(e.create());
  return FMD_OK;
}

/* what a blob of this geometry must look like: the create arguments and the designed sizes of the regions */
uint64_t state_fingerprint(const fmd_batch* b, const fmd_batch* x)
{
  uint64_t h = fnv1a("fmd-state", 9);
  auto mix = [&](const void* p, size_t n) { h = fnv1a(p, n, h); };
  const fmd_params& c = b->cparams;
  mix(&c.sample_rate_if, sizeof(double));
  mix(&c.tuning_offset, sizeof(double));
  mix(&c.sample_rate_pcm, sizeof(double));
  mix(&c.bandwidth_pcm, sizeof(double));
  mix(&c.downsample, sizeof(unsigned));
  mix(&c.us_version, sizeof(int));
  mix(&c.table_size, sizeof(unsigned));
  mix(&c.if_filter_order, sizeof(unsigned));
  mix(&c.fir_reduction, sizeof(int));
  for (int i = 0; i < x->state_tab.n; i++)
  {
    const fmd::StateRegion& r = x->state_tab.r[i];
    const uint64_t w[4] = {uint64_t(x->state_group[i]), r.rows, r.esz, r.off};
    mix(w, sizeof(w));
  }
  const uint64_t tail[4] = {gdec_bytes(), sizeof(StateHostRec), kOscBytes, sizeof(StateHeader)};
  mix(tail, sizeof(tail));
  return h;
}

StateClock clock_of(const fmd_batch* x)
{
  StateClock k{};
  k.if_pos = x->if_pos;
  k.lut_idx = x->lut_idx;
  k.rs_pos = x->rs_pos;
  k.rds_lpf_g = x->rds_lpf_g;
  k.mf_g = x->mf_g;
  k.alpf_g = x->alpf_g;
  k.hist_sel = x->hist_sel;
  k.call_index = x->call_index;
  k.osc_re = x->osc_on ? x->osc_re : 1.0f;
  k.osc_im = x->osc_on ? x->osc_im : 0.0f;
  k.lastM = x->lastM;
  k.lastA = x->lastA;
  k.lastR = x->lastR;
  return k;
}

/* the blob's sections */
struct StateView
{
  const StateHeader* h = nullptr;
  const char* osc = nullptr;
  const char* recs = nullptr;
  const char* payload = nullptr;
  const char* twin = nullptr;
};

size_t blob_bytes(size_t per_channel, unsigned n, bool twin)
{
  return sizeof(StateHeader) + kOscBytes + size_t(n) * host_rec_bytes() + size_t(n) * per_channel +
         (twin ? per_channel : 0);
}

/* checksum, build, geometry: everything a blob must pass before anything is touched */
int check_blob(fmd_batch* b, const void* blob, size_t size, const char* who, StateView* v)
{
  fmd_batch* x0 = first_part(b);
  StateHeader h;
  std::memcpy(&h, blob, sizeof(h));
  const std::string w(who);
  if (h.magic != kStateMagic || h.layout != kStateLayout || h.header_bytes != sizeof(StateHeader))
    return fail(FMD_ERR_ARG, w + ": not a state blob of this library (magic / layout version)");
  if (h.total_bytes != size)
    return fail(FMD_ERR_ARG, w + ": the blob is " + std::to_string(size) + " bytes, its header says " +
                                 std::to_string(h.total_bytes) + " (truncated?)");
  {
    StateHeader z = h;
    z.checksum = 0;
    uint64_t sum = fnv1a(&z, sizeof(z));
    sum = fnv1a(static_cast<const char*>(blob) + sizeof(z), size - sizeof(z), sum);
    if (sum != h.checksum)
      return fail(FMD_ERR_ARG, w + ": the blob's checksum does not match its contents");
  }
  char ver[sizeof(h.version)] = {};
  std::strncpy(ver, fmd_version(), sizeof(ver) - 1);
  if (std::memcmp(ver, h.version, sizeof(ver)) != 0)
    return fail(FMD_ERR_ARG, w + ": the blob was written by another build of the library (" +
                                 std::string(h.version, strnlen(h.version, sizeof(h.version))) + ")");
  if (h.fingerprint != state_fingerprint(b, x0))
    return fail(FMD_ERR_ARG, w + ": the blob is of another geometry (fmd_params or designed sizes differ)");
  if (h.n_channels == 0 || size != blob_bytes(x0->state_bytes, h.n_channels, (h.flags & SF_TWIN) != 0))
    return fail(FMD_ERR_ARG, w + ": the blob's size does not fit its channel count");
  const char* p = static_cast<const char*>(blob);
  v->h = reinterpret_cast<const StateHeader*>(p);
  v->osc = p + sizeof(StateHeader);
  v->recs = v->osc + kOscBytes;
  v->payload = v->recs + size_t(h.n_channels) * host_rec_bytes();
  v->twin = (h.flags & SF_TWIN) ? v->payload + size_t(h.n_channels) * x0->state_bytes : nullptr;
  return FMD_OK;
}

/* edits made and not yet applied by a call */
bool edits_waiting(fmd_batch* b)
{
  if (b->edits_pending)
    return true;
  for (const Part& p : parts(b))
    if (!p.x->edits.empty() || !p.x->imports.empty() || (p.x->map_on && p.x->map_dirty))
      return true;
  return false;
}

/* every call submitted so far is complete, on whatever stream it ran */
int drain_batch(fmd_batch* b)
{
  HIPCHK(hipSetDevice(b->device));
  if (int rc = wait_impl(b, 0, nullptr, false); rc < 0)
    return rc;
  HIPCHK(hipDeviceSynchronize());
  return check_device_errors(b);
}

/* the group decoder channel c continues with behind every call submitted so far (the one an edit still has to
 * reset, replace or bring in included); *fresh: 1 a reset one, 2 a new one (gdec_edit_between) */
const fmd::GroupDecoder* effective_gdec(fmd_batch* b, unsigned c, int* fresh)
{
  *fresh = 0;
  const fmd::GroupDecoder* g = b->gdec[c].get();
  uint32_t epoch = c < b->gdec_epoch.size() ? b->gdec_epoch[c] : 0u;
  if (auto it = b->gdec_imports.find(c); it != b->gdec_imports.end() && !it->second.empty())
  {
    g = it->second.back().g.get();
    epoch = std::max(epoch, it->second.back().k);
  }
  uint32_t k_last = 0;
  *fresh = gdec_edit_between(b, c, epoch, ~0u, &k_last);
  return *fresh == 2 ? nullptr : g;
}

/* header, oscillator entries and host records of the listed channels (null: all) of b into blob; the payload's
 * place is returned in *payload_at */
void write_host_part(fmd_batch* b, const unsigned* channels, unsigned n, uint32_t flags, char* blob, size_t total,
                     size_t* payload_at)
{
  fmd_batch* x0 = first_part(b);
  std::memset(blob, 0, sizeof(StateHeader) + kOscBytes + size_t(n) * host_rec_bytes());
  StateHeader h{};
  h.magic = kStateMagic;
  h.layout = kStateLayout;
  h.header_bytes = sizeof(StateHeader);
  std::strncpy(h.version, fmd_version(), sizeof(h.version) - 1);
  h.fingerprint = state_fingerprint(b, x0);
  h.n_channels = n;
  h.clock = clock_of(x0);
  h.cpc = b->cpc;
  h.n_cap = b->map_on ? b->n_cap : 0;
  h.total_bytes = total;
  bool origins = false;
  for (const Part& p : parts(b))
    origins = origins || p.x->origins_live;
  h.flags = flags | (origins ? SF_ORIGINS : 0u) | (x0->osc_on ? SF_OSC : 0u) | (b->map_on ? SF_MAP : 0u);
  char* p = blob + sizeof(StateHeader);
  if (x0->osc_on && x0->h_osc.p) // what the next call copies in front of its own entries (upload_oscillator)
    std::memcpy(p, x0->h_osc.p + size_t(x0->call_index % fmd_batch::NSLOT) * x0->h_osc_stride + x0->lastM, kOscBytes);
  p += kOscBytes;
  for (unsigned i = 0; i < n; i++, p += host_rec_bytes())
  {
    const unsigned c = channels ? channels[i] : i;
    StateHostRec r{};
    r.shift = shift_at(b, c, 0xffffffffu);
    r.capture = capture_at(b, c);
    unsigned lc = 0;
    const fmd_batch* ob = owner_of(b, c, &lc);
    unsigned w[fmd::HS_WORDS] = {};
    (void)host_status_read(ob, lc, w); // (no call in flight: never torn)
    std::memcpy(r.status, w, sizeof(w));
    int fresh = 0;
    const fmd::GroupDecoder* g = effective_gdec(b, c, &fresh);
    r.has_gdec = g ? 1u : 0u;
    std::memcpy(p, &r, sizeof(r));
    if (g)
    {
      fmd::GroupDecoder copy = *g;
      if (fresh)
        copy.reset();
      char* q = p + sizeof(r);
      copy.each_field([&](void* f, size_t k) {
        std::memcpy(q, f, k);
        q += k;
      });
    }
  }
  std::memcpy(blob, &h, sizeof(h));
  *payload_at = size_t(p - blob);
}

void seal_blob(char* blob, size_t total)
{
  StateHeader h;
  std::memcpy(&h, blob, sizeof(h));
  h.checksum = 0;
  std::memcpy(blob, &h, sizeof(h));
  h.checksum = fnv1a(blob, total);
  std::memcpy(blob, &h, sizeof(h));
}

unsigned state_blocks(unsigned n_list)
{ // a few channels: one workgroup per region; all channels: ~8 rows of every region per workgroup and pass
  return std::min(64u, (n_list * 8u + 255u) / 256u);
}

/* the regions a load or import writes: all but the skipped group's */
fmd::StateTable table_without(const fmd_batch* x, int skip)
{
  fmd::StateTable t{};
  for (int i = 0; i < x->state_tab.n; i++)
    if (x->state_group[i] != skip)
      t.r[t.n++] = x->state_tab.r[i];
  return t;
}

/* the listed channels (null: all) of b, packed into dev[0 .. n * state_bytes): one launch per batch with buffers */
int export_payload(fmd_batch* b, const unsigned* channels, unsigned n, char* dev)
{
  DevBuf<fmd::StateEdit> d_list;
  std::vector<fmd::StateEdit> list;
  for (const auto& [x, ch0] : parts(b))
  {
    if (!channels)
    {
      hipLaunchKernelGGL(fmd::k_channel_export, dim3(state_blocks(x->C), x->state_tab.n), dim3(256), 0, nullptr,
                         x->state_tab, (const fmd::StateEdit*)nullptr, x->C, (void*)dev, n, ch0);
      continue;
    }
    list.clear();
    for (unsigned i = 0; i < n; i++)
      if (channels[i] >= ch0 && channels[i] - ch0 < x->C)
        list.push_back(fmd::StateEdit{int(channels[i] - ch0), int(i), 0, 0});
    if (list.empty())
      continue;
    if (d_list.alloc(list.size()) || upload(d_list.p, list.data(), list.size() * sizeof(fmd::StateEdit)))
      return fail(FMD_ERR_DEVICE, "fmd_batch_export_channels: device allocation failed");
    hipLaunchKernelGGL(fmd::k_channel_export, dim3(state_blocks(unsigned(list.size())), x->state_tab.n), dim3(256), 0,
                       nullptr, x->state_tab, (const fmd::StateEdit*)d_list.p, unsigned(list.size()), (void*)dev, n, 0u);
    HIPCHK(hipDeviceSynchronize()); // (the list is freed or reused next)
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  return FMD_OK;
}

int save_impl(fmd_batch* b, const unsigned* channels, unsigned n, void* blob, size_t cap, size_t* written,
              const char* who)
{
  const std::string w(who);
  if (b->failed)
    return fail(FMD_ERR_ARG, w + ": the batch has failed (fmd_batch_reset clears it)");
  if (edits_waiting(b))
    return fail(FMD_ERR_STATE, w + ": edits are pending (a retune, reset, capture switch or import that no call has "
                                   "applied yet): make the next call first");
  if (int rc = drain_batch(b))
    return rc;
  for (const Part& p : parts(b))
    if (int rc = ensure_state_table(p.x))
      return rc;
  const bool whole = channels == nullptr;
  fmd_batch* tw = whole ? b->twin.get() : nullptr;
  if (tw)
    if (int rc = ensure_state_table(tw))
      return rc;
  const size_t per = first_part(b)->state_bytes;
  const size_t total = blob_bytes(per, n, tw != nullptr);
  if (written)
    *written = total;
  if (cap < total)
    return fail(FMD_ERR_ARG, w + ": the buffer takes " + std::to_string(cap) + " bytes, the state " +
                                 std::to_string(total) + " (fmd_batch_state_size)");
  char* out = static_cast<char*>(blob);
  size_t at = 0;
  write_host_part(b, channels, n, (whole ? SF_WHOLE : 0u) | (tw ? SF_TWIN : 0u), out, total, &at);
  DevBuf<char> dev;
  if (dev.alloc(size_t(n) * per + per))
    return fail(FMD_ERR_DEVICE, w + ": device allocation failed");
  if (int rc = export_payload(b, channels, n, dev.p))
    return rc;
  if (tw)
  {
    hipLaunchKernelGGL(fmd::k_channel_export, dim3(1, tw->state_tab.n), dim3(256), 0, nullptr, tw->state_tab,
                       (const fmd::StateEdit*)nullptr, 1u, (void*)(dev.p + size_t(n) * per), 1u, 0u);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpy(out + at, dev.p, total - at, hipMemcpyDeviceToHost));
  seal_blob(out, total);
  return FMD_OK;
}

/* The host's copy of one channel's status snapshot (fmd::HostStatusWord's protocol).  The write is opened with a
 * tag of the host's own (host_seq: no call index and no earlier host write has it), so a getter that reads while
 * the words change finds BEGIN != END whatever tags the old record and the blob's carry -- they may be the same,
 * a standby at the source's call index for one.  The recorded tags go in last, BEGIN then END: a reader that takes
 * the new END has every word (it reads END first), one that still takes the old END finds BEGIN changed. */
void host_status_put(fmd_batch* x, unsigned c, const uint32_t* w)
{
  const size_t CP = x->CP;
  unsigned* h = x->h_status.p + c;
  __atomic_store_n(&h[fmd::HS_SEQ_BEGIN * CP], 0x80000000u | ++x->host_seq, __ATOMIC_RELEASE);
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  for (int i = fmd::HS_SEQ_BEGIN + 1; i < fmd::HS_SEQ_END; i++)
    __atomic_store_n(&h[size_t(i) * CP], w[i], __ATOMIC_RELAXED);
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  __atomic_store_n(&h[fmd::HS_SEQ_BEGIN * CP], w[fmd::HS_SEQ_BEGIN], __ATOMIC_RELEASE);
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  __atomic_store_n(&h[fmd::HS_SEQ_END * CP], w[fmd::HS_SEQ_END], __ATOMIC_RELEASE);
}

std::unique_ptr<fmd::GroupDecoder> gdec_from_rec(fmd_batch* b, unsigned c, const char* rec)
{
  StateHostRec r;
  std::memcpy(&r, rec, sizeof(r));
  if (!r.has_gdec)
    return nullptr;
  std::unique_ptr<fmd::GroupDecoder> g(new fmd::GroupDecoder(&b->cb, b->user, c));
  const char* q = rec + sizeof(r);
  g->each_field([&](void* f, size_t k) {
    std::memcpy(f, q, k);
    q += k;
  });
  return g;
}

/* the batch-uniform words of a batch with buffers of its own, from a blob's clock */
void take_clock(fmd_batch* x, const StateView& v)
{
  const StateClock& k = v.h->clock;
  x->if_pos = k.if_pos;
  x->lut_idx = k.lut_idx;
  x->rs_pos = k.rs_pos;
  x->rds_lpf_g = k.rds_lpf_g;
  x->mf_g = k.mf_g;
  x->alpf_g = k.alpf_g;
  x->hist_sel = k.hist_sel;
  __atomic_store_n(&x->call_index, k.call_index, __ATOMIC_RELAXED); // (fmd_batch_get_status reads it from any thread)
  x->lastM = k.lastM;
  x->lastA = k.lastA;
  x->lastR = k.lastR;
  x->origins_live = (v.h->flags & SF_ORIGINS) != 0;
  std::memset(x->slot_call, 0, sizeof(x->slot_call));
  std::memset(x->drained_call, 0, sizeof(x->drained_call));
  x->osc_warm = 0;
  if (x->osc_on && x->h_osc.p)
  {
    if (v.h->flags & SF_OSC)
    {
      x->osc_re = k.osc_re;
      x->osc_im = k.osc_im;
      std::memcpy(x->h_osc.p + size_t(k.call_index % fmd_batch::NSLOT) * x->h_osc_stride + k.lastM, v.osc, kOscBytes);
    }
    else
      x->osc_warm = fmd_batch::kOscH; // (osc_re / osc_im: from channel 0's state, see load_impl)
  }
}

/* the second half of a load: every write (load_impl has checked the blob and staged the payload at dev) */
int load_replace(fmd_batch* b, const StateView& v, char* dev_p, const char* who)
{
  const std::vector<Part> ps = parts(b);
  const size_t per = ps[0].x->state_bytes;
  const int skip = b->state_skip;
  const unsigned T = b->des.table_size;
  b->gdec_imports.clear();
  b->edits_pending = false;
  {
    std::lock_guard<std::mutex> lk(b->log_mu);
    for (auto& log : b->shift_log)
      log.clear();
    for (auto& log : b->retune_log)
      log.clear();
  }
  std::fill(b->gdec_epoch.begin(), b->gdec_epoch.end(), 0u);
  for (const auto& [x, ch0] : ps)
  {
    const fmd::StateTable tab = table_without(x, skip);
    hipLaunchKernelGGL(fmd::k_channel_import, dim3(state_blocks(x->C), tab.n + 1), dim3(256), 0, nullptr, tab,
                       (const fmd::StateEdit*)nullptr, x->C, (const void*)dev_p, b->C, ch0, (const float2*)nullptr,
                       (float2*)x->lut.p, T);
    HIPCHK(hipGetLastError());
    // tuner rows: rebuilt from the shifts, as the batch's creation does
    std::vector<float> lut(size_t(2) * T * x->C);
    for (unsigned c = 0; c < x->C; c++)
    {
      StateHostRec r;
      std::memcpy(&r, v.recs + size_t(ch0 + c) * host_rec_bytes(), sizeof(r));
      { // (the getters read the shift from any thread, under the log's mutex: shift_at)
        std::lock_guard<std::mutex> lk(b->log_mu);
        x->shifts[c] = r.shift;
        b->shifts[ch0 + c] = r.shift;
      }
      if (c > 0 && x->shifts[c] == x->shifts[c - 1])
        std::copy_n(&lut[size_t(2) * T * (c - 1)], 2 * T, &lut[size_t(2) * T * c]);
      else
      {
        const auto t = fmd::make_tuner_lut(T, r.shift);
        std::copy(t.begin(), t.end(), &lut[size_t(2) * T * c]);
      }
      if (skip != kSkipStatus)
        host_status_put(x, c, r.status);
      if (skip != kSkipGdec)
        b->gdec[ch0 + c] = gdec_from_rec(b, ch0 + c, v.recs + size_t(ch0 + c) * host_rec_bytes());
    }
    if (upload(x->lut.p, lut.data(), lut.size() * sizeof(float)))
      return fail(FMD_ERR_DEVICE, std::string(who) + ": upload of the tuner tables failed");
    x->edits.clear();
    x->imports.clear();
    take_clock(x, v);
    HIPCHK(hipMemset(x->groups.counts.p, 0, fmd_batch::NSLOT * sizeof(unsigned))); // queued groups are dropped
    if (x->blocks.counts.p) // ... and queued block records (the counters of the observation stay: not the decoder's)
    {
      HIPCHK(hipMemset(x->blocks.counts.p, 0, fmd_batch::NSLOT * sizeof(unsigned)));
      std::memset(x->rb_dirty, 0, sizeof(x->rb_dirty));
    }
    if (x->h_err.p)
    {
      __atomic_store_n(&x->h_err.p[0], 0u, __ATOMIC_RELEASE);
      __atomic_store_n(&x->h_err.p[1], 0u, __ATOMIC_RELEASE);
    }
    x->failed = false;
    x->fail_msg.clear();
  }
  if (fmd_batch* tw = b->twin.get())
  {
    const fmd::StateTable tab = table_without(tw, skip);
    hipLaunchKernelGGL(fmd::k_channel_import, dim3(1, tab.n + 1), dim3(256), 0, nullptr, tab,
                       (const fmd::StateEdit*)nullptr, 1u, (const void*)(dev_p + size_t(b->C) * per), 1u, 0u,
                       (const float2*)nullptr, (float2*)tw->lut.p, T);
    HIPCHK(hipGetLastError());
    take_clock(tw, v);
    tw->edits.clear();
    tw->failed = false;
    tw->fail_msg.clear();
  }
  HIPCHK(hipDeviceSynchronize());
  // a destination that keeps the oscillator sequence where the source did not: the sequence's state is every
  // channel's own copy of it (k_demod_serial leaves it in F_OSC_RE / F_OSC_IM in either form)
  for (const Part& p : ps)
    if (p.x->osc_warm)
    {
      HIPCHK(hipMemcpy(&p.x->osc_re, p.x->st.F(fmd::F_OSC_RE), sizeof(float), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(&p.x->osc_im, p.x->st.F(fmd::F_OSC_IM), sizeof(float), hipMemcpyDeviceToHost));
    }
  // the capture map as the next call reads it
  if (v.h->flags & SF_MAP)
  {
    set_all(b, &fmd_batch::cpc, 1u);
    if (int rc = ensure_map(b, who))
      return rc;
    for (const auto& [x, ch0] : ps)
    {
      for (unsigned c = 0; c < x->C; c++)
      {
        StateHostRec r;
        std::memcpy(&r, v.recs + size_t(ch0 + c) * host_rec_bytes(), sizeof(r));
        x->cmap[c] = r.capture;
      }
      x->map_dirty = true; // (part of the load: the next call uploads the walk like any call behind a switch)
    }
    set_all(b, &fmd_batch::n_cap, v.h->n_cap);
  }
  else
  {
    set_all(b, &fmd_batch::cpc, v.h->cpc);
    set_all(b, &fmd_batch::map_on, false);
    set_all(b, &fmd_batch::n_cap, 0u);
    for (const Part& p : ps)
      p.x->map_dirty = false;
  }
  if (is_shell(b))
  {
    const fmd_batch* x0 = ps[0].x;
    __atomic_store_n(&b->call_index, x0->call_index, __ATOMIC_RELAXED);
    b->lastM = x0->lastM;
    b->lastA = x0->lastA;
    b->lastR = x0->lastR;
  }
  b->failed = false;
  b->fail_msg.clear();
  return FMD_OK;
}

int load_impl(fmd_batch* b, const void* blob, size_t size)
{
  const char* who = "fmd_batch_load_state";
  HIPCHK(hipSetDevice(b->device));
  for (const Part& p : parts(b))
    if (int rc = ensure_state_table(p.x))
      return rc;
  if (b->twin)
    if (int rc = ensure_state_table(b->twin.get()))
      return rc;
  StateView v;
  if (int rc = check_blob(b, blob, size, who, &v))
    return rc;
  if (!(v.h->flags & SF_WHOLE))
    return fail(FMD_ERR_ARG, std::string(who) + ": the blob holds exported channels, not a whole batch "
                                                "(fmd_batch_import_channels takes it)");
  if (v.h->n_channels != b->C)
    return fail(FMD_ERR_ARG, std::string(who) + ": the blob holds " + std::to_string(v.h->n_channels) +
                                 " channels, the batch " + std::to_string(b->C));
  if (((v.h->flags & SF_TWIN) != 0) != (b->twin != nullptr))
    return fail(FMD_ERR_STATE, std::string(who) + ((v.h->flags & SF_TWIN)
                                                       ? ": the saved batch had retuning enabled, this one has not "
                                                         "(fmd_batch_enable_retune before the first call)"
                                                       : ": this batch has retuning enabled, the saved one had not"));
  if (!(v.h->flags & SF_MAP) && (v.h->cpc == 0 || b->C % v.h->cpc))
    return fail(FMD_ERR_ARG, std::string(who) + ": the blob's channels per capture do not divide the channel count");
  (void)wait_impl(b, 0, nullptr, false); // (a failed batch may be loaded into)
  HIPCHK(hipDeviceSynchronize());
  const size_t per = first_part(b)->state_bytes;
  DevBuf<char> dev;
  if (dev.alloc(size_t(b->C) * per + per))
    return fail(FMD_ERR_DEVICE, std::string(who) + ": device allocation failed");
  HIPCHK(hipMemcpy(dev.p, v.payload, size_t(b->C) * per + (v.twin ? per : 0), hipMemcpyHostToDevice));
  // ---- nothing of the batch was touched so far; from here on it is replaced.  A step that fails now leaves it
  // neither the old batch nor the blob's: it refuses further calls until a load or fmd_batch_reset succeeds ----
  const int rc = load_replace(b, v, dev.p, who);
  if (rc != FMD_OK)
  {
    const std::string why = g_err;
    b->failed = true;
    b->fail_msg = std::string(who) + " broke off half-way (" + why + "): load again or reset the batch";
    return fail(rc, b->fail_msg);
  }
  return FMD_OK;
}
/* the first batch-uniform word in which a blob's clock differs from the batch's in front of its next call */
const char* clock_difference(const fmd_batch* x, const StateView& v)
{
  const StateClock a = clock_of(x);
  const StateClock& k = v.h->clock;
  if (a.if_pos != k.if_pos)
    return "if_pos (the IF decimator's phase)";
  if (a.lut_idx != k.lut_idx)
    return "lut_idx (the tuner table's index)";
  if (std::memcmp(&a.rs_pos, &k.rs_pos, sizeof(float)) != 0)
    return "rs_pos (the resampler's fractional position)";
  if (a.rds_lpf_g != k.rds_lpf_g)
    return "rds_lpf_g (the RDS low-pass ring's phase)";
  if (a.mf_g != k.mf_g)
    return "mf_g (the matched filter ring's phase)";
  if (a.alpf_g != k.alpf_g)
    return "alpf_g (the audio low-pass ring's phase)";
  if (a.hist_sel != k.hist_sel)
    return "hist_sel (the IF history's ping-pong)";
  if ((a.call_index & 3u) != (k.call_index & 3u))
    return "call_index (buffer parity: the call indices differ mod 4)";
  if (x->osc_on && (v.h->flags & SF_OSC) &&
      (std::memcmp(&a.osc_re, &k.osc_re, sizeof(float)) != 0 || std::memcmp(&a.osc_im, &k.osc_im, sizeof(float)) != 0))
    return "osc_re / osc_im (the RDS oscillator sequence)";
  return nullptr;
}

int import_impl(fmd_batch* b, const unsigned* channels, unsigned n, const void* blob, size_t size)
{
  const char* who = "fmd_batch_import_channels";
  if (int rc = check_channel_list(b, channels, nullptr, n, who))
    return rc;
  HIPCHK(hipSetDevice(b->device));
  const std::vector<Part> ps = parts(b);
  for (const Part& p : ps)
    if (int rc = ensure_state_table(p.x))
      return rc;
  StateView v;
  if (int rc = check_blob(b, blob, size, who, &v))
    return rc;
  if (v.h->n_channels != n)
    return fail(FMD_ERR_ARG, std::string(who) + ": the blob holds " + std::to_string(v.h->n_channels) +
                                 " channels, the list names " + std::to_string(n));
  if (const char* word = clock_difference(ps[0].x, v))
    return fail(FMD_ERR_STATE, std::string(who) + ": the blob's clock differs from the batch's in front of its next "
                                                  "call, first in " + word +
                                   ": a decoder continues only in a batch fed the same sequence of call sizes");
  const unsigned T = b->des.table_size;
  const size_t per = ps[0].x->state_bytes;
  // ---- per batch with buffers: its channels of the list, sorted, and the tuner rows they need ----
  struct Plan
  {
    fmd_batch* x;
    fmd_batch::PendingImport p;
    std::vector<int> row_shift;
  };
  std::vector<Plan> plans;
  for (const auto& [x, ch0] : ps)
  {
    Plan pl{x, {}, {}};
    std::map<int, int> row_of;
    for (unsigned i = 0; i < n; i++)
    {
      if (channels[i] < ch0 || channels[i] - ch0 >= x->C)
        continue;
      StateHostRec r;
      std::memcpy(&r, v.recs + size_t(i) * host_rec_bytes(), sizeof(r));
      const int s = int((long long)(r.shift) % (long long)T); // (a row depends on the remainder: submit_edits)
      auto it = row_of.find(s);
      if (it == row_of.end())
      {
        it = row_of.emplace(s, int(pl.row_shift.size())).first;
        pl.row_shift.push_back(s);
      }
      pl.p.list.push_back(fmd::StateEdit{int(channels[i] - ch0), int(i), it->second, 0});
    }
    if (pl.p.list.empty())
      continue;
    std::sort(pl.p.list.begin(), pl.p.list.end(),
              [](const fmd::StateEdit& a, const fmd::StateEdit& z) { return a.ch < z.ch; });
    if (x->imports.size() >= size_t(fmd_batch::NSLOT))
      return fail(FMD_ERR_STATE, std::string(who) + ": eight imports are waiting for the batch's next call");
    pl.p.n_cols = n;
    pl.p.n_rows = unsigned(pl.row_shift.size());
    pl.p.rows_at = (pl.p.list.size() * sizeof(fmd::StateEdit) + 15) & ~size_t(15);
    pl.p.payload_at = (pl.p.rows_at + size_t(pl.p.n_rows) * T * sizeof(float2) + 15) & ~size_t(15);
    pl.p.bytes = pl.p.payload_at + size_t(n) * per;
    pl.p.origins_live = (v.h->flags & SF_ORIGINS) != 0;
    plans.push_back(std::move(pl));
  }
  // ---- staging: a page-locked slot and a device slot in rotation, sized on first use ----
  for (Plan& pl : plans)
  {
    fmd_batch* x = pl.x;
    const int slot = int(x->imp_seq++ % fmd_batch::NSLOT);
    HIPCHK(x->imp_ev[slot].sync_if_in_use()); // the copy of eight imports ago
    if (x->h_imp[slot].n < pl.p.bytes || x->d_imp[slot].n < pl.p.bytes)
    { // (growing a slot frees the old one: the runtime waits for whatever still reads it)
      const size_t want = std::max(pl.p.bytes, size_t(1) << 16);
      if (x->h_imp[slot].alloc(want) || x->d_imp[slot].alloc(want))
        return fail(FMD_ERR_DEVICE, std::string(who) + ": staging allocation failed");
    }
    pl.p.slot = slot;
    char* h = x->h_imp[slot].p;
    for (unsigned r = 0; r < pl.p.n_rows; r++)
    {
      const auto lut = fmd::make_tuner_lut(T, pl.row_shift[r]);
      std::memcpy(h + pl.p.rows_at + size_t(r) * T * sizeof(float2), lut.data(), size_t(T) * sizeof(float2));
    }
    std::memcpy(h + pl.p.payload_at, v.payload, size_t(n) * per);
  }
  // ---- the edit itself: nothing can fail from here on ----
  const uint32_t k = b->call_index + 1; // the call the edit takes effect at
  std::lock_guard<std::mutex> lk(b->log_mu);
  if (b->shift_log.empty())
  {
    b->shift_log.resize(b->C);
    b->gdec_epoch.assign(b->C, 0u);
  }
  for (Plan& pl : plans)
  {
    fmd_batch* x = pl.x;
    const int index = int(x->imports.size());
    for (const fmd::StateEdit& e : pl.p.list)
    {
      StateHostRec r;
      std::memcpy(&r, v.recs + size_t(e.col) * host_rec_bytes(), sizeof(r));
      x->edits.push_back(fmd_batch::Edit{unsigned(e.ch), r.shift, false, index});
    }
    x->imports.push_back(std::move(pl.p));
  }
  for (unsigned i = 0; i < n; i++)
  {
    const unsigned c = channels[i];
    StateHostRec r;
    std::memcpy(&r, v.recs + size_t(i) * host_rec_bytes(), sizeof(r));
    auto& log = b->shift_log[c];
    if (!log.empty() && log.back().first == k)
      log.back().second = r.shift;
    else
      log.emplace_back(k, r.shift);
    if (b->state_skip != kSkipGdec)
    {
      auto& pend = b->gdec_imports[c];
      while (!pend.empty() && pend.back().k >= k)
        pend.pop_back();
      pend.push_back(fmd_batch::GdecImport{k, gdec_from_rec(b, c, v.recs + size_t(i) * host_rec_bytes())});
    }
  }
  b->edits_pending = true;
  return FMD_OK;
}

/* The imports waiting in x, on the IF stage's stream behind every earlier call (submit_edits): per import the
 * channels that still end up with it (import_of: channel -> entry of x->imports), one copy of its staging slot and
 * one launch. */
int submit_imports(fmd_batch* x, hipStream_t sF, const std::map<unsigned, int>& import_of)
{
  const unsigned T = x->des.table_size;
  for (size_t i = 0; i < x->imports.size(); i++)
  {
    fmd_batch::PendingImport& p = x->imports[i];
    fmd::StateEdit* hl = reinterpret_cast<fmd::StateEdit*>(x->h_imp[p.slot].p);
    unsigned m = 0;
    for (const fmd::StateEdit& e : p.list)
    {
      auto it = import_of.find(unsigned(e.ch));
      if (it != import_of.end() && it->second == int(i))
        hl[m++] = e;
    }
    if (m == 0)
      continue;
    char* d = x->d_imp[p.slot].p;
    HIPCHK(hipMemcpyAsync(d, x->h_imp[p.slot].p, p.bytes, hipMemcpyHostToDevice, sF));
    HIPCHK(x->imp_ev[p.slot].record_use(sF));
    const fmd::StateTable tab = table_without(x, x->state_skip);
    hipLaunchKernelGGL(fmd::k_channel_import, dim3(state_blocks(m), tab.n + 1), dim3(256), 0, sF, tab,
                       (const fmd::StateEdit*)d, m, (const void*)(d + p.payload_at), p.n_cols, 0u,
                       (const float2*)(d + p.rows_at), (float2*)x->lut.p, T);
    HIPCHK(hipGetLastError());
    if (p.origins_live)
      x->origins_live = true;
  }
  x->imports.clear();
  return FMD_OK;
}

} // namespace

extern "C" {

size_t fmd_batch_state_size(const fmd_batch* b, unsigned n_channels)
{
  if (!b || n_channels == 0)
    return 0;
  fmd_batch* m = const_cast<fmd_batch*>(b);
  if (hipSetDevice(b->device) != hipSuccess)
    return 0;
  for (const Part& p : parts(m))
    if (ensure_state_table(p.x))
      return 0;
  return blob_bytes(first_part(m)->state_bytes, n_channels, n_channels == b->C && b->twin != nullptr);
}

int fmd_batch_save_state(fmd_batch* b, void* blob, size_t cap, size_t* written)
{
  if (!b || !blob)
    return fail(FMD_ERR_ARG, "fmd_batch_save_state: null argument");
  if (cap < sizeof(StateHeader))
    return fail(FMD_ERR_ARG, "fmd_batch_save_state: the buffer is smaller than a blob's header");
  return save_impl(b, nullptr, b->C, blob, cap, written, "fmd_batch_save_state");
}

int fmd_batch_load_state(fmd_batch* b, const void* blob, size_t size)
{
  if (!b || !blob)
    return fail(FMD_ERR_ARG, "fmd_batch_load_state: null argument");
  if (size < sizeof(StateHeader))
    return fail(FMD_ERR_ARG, "fmd_batch_load_state: the blob is smaller than a blob's header");
  return load_impl(b, blob, size);
}

int fmd_batch_export_channels(fmd_batch* b, const unsigned* channels, unsigned n, void* blob, size_t cap,
                              size_t* written)
{
  if (!b || !channels || !blob)
    return fail(FMD_ERR_ARG, "fmd_batch_export_channels: null argument");
  if (cap < sizeof(StateHeader))
    return fail(FMD_ERR_ARG, "fmd_batch_export_channels: the buffer is smaller than a blob's header");
  if (n == 0)
    return fail(FMD_ERR_ARG, "fmd_batch_export_channels: no channels");
  if (int rc = check_channel_list(b, channels, nullptr, n, "fmd_batch_export_channels"))
    return rc;
  return save_impl(b, channels, n, blob, cap, written, "fmd_batch_export_channels");
}

int fmd_batch_import_channels(fmd_batch* b, const unsigned* channels, unsigned n, const void* blob, size_t size)
{
  if (!b || !channels || !blob)
    return fail(FMD_ERR_ARG, "fmd_batch_import_channels: null argument");
  if (size < sizeof(StateHeader))
    return fail(FMD_ERR_ARG, "fmd_batch_import_channels: the blob is smaller than a blob's header");
  return import_impl(b, channels, n, blob, size);
}

int fmd_save_state(fmd_decoder* d, void* blob, size_t cap, size_t* written)
{
  if (!d || !blob)
    return fail(FMD_ERR_ARG, "fmd_save_state: null argument");
  return fmd_batch_save_state(d->b, blob, cap, written);
}

int fmd_load_state(fmd_decoder* d, const void* blob, size_t size)
{
  if (!d || !blob)
    return fail(FMD_ERR_ARG, "fmd_load_state: null argument");
  return fmd_batch_load_state(d->b, blob, size);
}

int fmd_batch_debug_state_skip(fmd_batch* b, int region)
{
  if (!b)
    return fail(FMD_ERR_ARG, "fmd_batch_debug_state_skip: null batch");
  if (region < -1 || region >= kSkipCount)
  {
    std::string names;
    for (const char* r : kRestartRegions)
      names += std::string(r) + ", ";
    return fail(FMD_ERR_ARG, "fmd_batch_debug_state_skip: -1 or the index of a region (" + names +
                                 "status record, group decoder, audio meter / clip counter)");
  }
  set_all(b, &fmd_batch::state_skip, region);
  if (b->twin)
    b->twin->state_skip = region;
  return FMD_OK;
}

} // extern "C"
