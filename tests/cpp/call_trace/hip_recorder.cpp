/*
 * hip_recorder.cpp -- a recording double of the HIP runtime calls that the host object of csrc/fmd_batch.hip makes,
 * for tests/test_call_trace_cpu.py only.  Linked with that object and call_trace.cpp in place of libamdhip64: the
 * program never opens a GPU.
 *
 *  - "Device" memory is host memory (calloc), so the library's own host-side copies and memsets work.
 *  - Kernels are NOT run.  A launch becomes one text line: call form (launch / xlaunch), stream, kernel, grid, block,
 *    dynamic LDS and, for the ext form, its two events.  Event records, stream waits, the synchronising calls, copies
 *    and memsets (bytes, kind, stream) and hipFuncSetAttribute are lines too.
 *  - Streams and events are numbered by a counter when they are created (s1, s2, ...; e1, e2, ...; s0 is the null
 *    stream, e0 no event), never by pointer value: a handle that is freed and reused cannot alias.
 *  - Kernel names come from __hipRegisterFunction; the trace prints them demangled without the namespace and the
 *    parameter list; rec_kernels() prints the sorted list of every registered kernel in that form and mangled.
 *  - Kernel ARGUMENTS are not recorded: their sizes are not known to the double.  Which buffer a launch gets stays
 *    the business of the bit-exact GPU tests; this double pins which kernel goes to which stream, in which order,
 *    with which geometry, behind and in front of which events.
 *
 * Switches for the driver: rec_on(0 / 1) recording off / on; rec_epoch(): the numbering starts again (in front of
 * every fresh batch, so that equal schedules give equal text); rec_busy(1): "the caller's stream is busy, events have
 * not completed yet" -- hipStreamQuery and hipEventQuery answer hipErrorNotReady; rec_stream(): a numbered stream to
 * pass as the caller's.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <cxxabi.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

struct ihipStream_t
{
  int id;
};
struct ihipEvent_t
{
  int id;
};

namespace
{
bool g_on = false, g_busy = false;
int g_streams = 0, g_events = 0;
std::map<const void*, std::string>& names() // (filled by static initialisers of the object under test)
{
  static std::map<const void*, std::string> m;
  return m;
}
std::set<std::string>& mangled()
{
  static std::set<std::string> s;
  return s;
}
struct Cfg
{
  dim3 g, b;
  size_t lds;
  hipStream_t s;
};
std::vector<Cfg> g_cfg;
#define LOG(...) (void)(g_on && printf(__VA_ARGS__))

int sid(hipStream_t s) { return s ? s->id : 0; }
int eid(hipEvent_t e) { return e ? e->id : 0; }

/* "void fmd::k_roll<float>(float const*, ...)" -> "k_roll<float>" */
std::string short_name(const char* m)
{
  int st = 0;
  char* d = abi::__cxa_demangle(m, nullptr, nullptr, &st);
  std::string s = (st == 0 && d) ? d : m;
  free(d);
  int depth = 0;
  size_t cut = s.size();
  for (size_t i = 0; i < s.size(); i++)
  {
    if (s[i] == '<')
      depth++;
    else if (s[i] == '>')
      depth--;
    else if (s[i] == '(' && depth == 0)
    {
      cut = i;
      break;
    }
  }
  s.resize(cut);
  if (s.rfind("void ", 0) == 0)
    s.erase(0, 5);
  const char* const from[] = {"fmd::", "HIP_vector_type<float, 2u>", " >"};
  const char* const to[] = {"", "float2", ">"};
  for (int k = 0; k < 3; k++)
    for (size_t at; (at = s.find(from[k])) != std::string::npos;)
      s.replace(at, strlen(from[k]), to[k]);
  return s;
}

/* "128", "128,4" or "128,4,2": trailing ones are left out */
std::string dims(dim3 d)
{
  std::string s = std::to_string(d.x);
  if (d.y != 1 || d.z != 1)
    s += "," + std::to_string(d.y);
  if (d.z != 1)
    s += "," + std::to_string(d.z);
  return s;
}

void log_launch(const char* form, const void* f, dim3 g, dim3 b, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                bool ext)
{
  if (!g_on)
    return;
  auto it = names().find(f);
  printf("%s s%d %s grid %s block %s", form, sid(s), it == names().end() ? "?" : it->second.c_str(), dims(g).c_str(),
         dims(b).c_str());
  if (lds)
    printf(" lds %zu", lds);
  if (ext)
    printf(" ev e%d e%d", eid(e0), eid(e1));
  printf("\n");
}
} // namespace

extern "C"
{
void rec_on(int on) { g_on = on != 0; }
void rec_busy(int busy) { g_busy = busy != 0; }
void rec_epoch() { g_streams = g_events = 0; } // (a fresh batch, every older handle is gone: numbers start again)
void* rec_stream() { return new ihipStream_t{++g_streams}; }
void rec_kernels()
{
  std::set<std::string> shorts;
  for (const auto& n : names())
    shorts.insert(n.second);
  for (const std::string& n : shorts)
    printf("kernel %s\n", n.c_str());
  for (const std::string& m : mangled())
    printf("mangled %s\n", m.c_str());
}

void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* name, unsigned, void*, void*, void*, void*, int*)
{
  names()[host] = short_name(name);
  mangled().insert(name);
}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t lds, hipStream_t s)
{
  g_cfg.push_back({g, b, lds, s});
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* lds, hipStream_t* s)
{
  const Cfg c = g_cfg.back();
  g_cfg.pop_back();
  *g = c.g;
  *b = c.b;
  *lds = c.lds;
  *s = c.s;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t lds, hipStream_t s)
{
  log_launch("launch", f, g, b, lds, s, nullptr, nullptr, false);
  return hipSuccess;
}
hipError_t hipExtLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t lds, hipStream_t s, hipEvent_t e0,
                              hipEvent_t e1, int)
{
  log_launch("xlaunch", f, g, b, lds, s, e0, e1, true);
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute a, int v)
{
  if (g_on)
  {
    auto it = names().find(f);
    printf("funcattr %s %d %d\n", it == names().end() ? "?" : it->second.c_str(), int(a), v);
  }
  return hipSuccess;
}

hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) // (the header's macro gives this its versioned name)
{
  memset(p, 0, sizeof(*p));
  p->multiProcessorCount = 256;
  strcpy(p->gcnArchName, "gfx950");
  p->sharedMemPerBlock = 160 * 1024;
  p->maxSharedMemoryPerMultiProcessor = 160 * 1024;
  return hipSuccess;
}
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "error of the recording double"; }
hipError_t hipGetLastError() { return hipSuccess; }

hipError_t hipMalloc(void** p, size_t n) { *p = calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned)
{
  *p = calloc(1, n ? n : 1);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k)
{
  memcpy(d, s, n);
  LOG("memcpy %zu kind %d\n", n, int(k));
  return hipSuccess;
}
hipError_t hipMemcpy2D(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind k)
{
  for (size_t r = 0; r < h; r++)
    memcpy(static_cast<char*>(d) + r * dp, static_cast<const char*>(s) + r * sp, w);
  LOG("memcpy2d %zu x %zu kind %d\n", w, h, int(k));
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st)
{
  memmove(d, s, n);
  LOG("copy s%d %zu kind %d\n", sid(st), n, int(k));
  return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) { memset(d, v, n); LOG("memset %zu\n", n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st)
{
  memset(d, v, n);
  LOG("set s%d %zu\n", sid(st), n);
  return hipSuccess;
}

hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int)
{
  *s = new ihipStream_t{++g_streams};
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { delete s; return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t) { return g_busy ? hipErrorNotReady : hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { LOG("streamsync s%d\n", sid(s)); return hipSuccess; }
hipError_t hipDeviceSynchronize() { LOG("devicesync\n"); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
  LOG("wait s%d e%d\n", sid(s), eid(e));
  return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned)
{
  *e = new ihipEvent_t{++g_events};
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { delete e; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { LOG("record e%d s%d\n", eid(e), sid(s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { LOG("eventsync e%d\n", eid(e)); return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return g_busy ? hipErrorNotReady : hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }
}
