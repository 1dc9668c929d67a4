// kv_prefix.hip — the device prompt cache: rows [0, n) of one sequence's KV cache saved into, and restored from, one packed device
// buffer (lgh_prefix_*).  The device side of the reference's PromptCache / PrefixSharing (src/model/cache.rs:28-345), whose
// CachedPrefix clones the K / V tensors of every layer on the host.
//
// One call = ONE launch of kv_prefix_copy_kernel<RESTORE>, whatever the number of layers and tensors: a workgroup column per SEGMENT,
// a segment = the n positions of one kv head of one tensor (KvKind) of one owned layer:
//   cache    n * pos_bytes contiguous bytes at ((slot * n_kv + h) * max_seq) * pos_bytes of the layer's tensor (kv_cache.h)
//   packed   [layer][kind the format has][kv head][n_stride][pos_bytes], no padding between segments
//            (n_stride = the rows the buffer was saved with; a restore may copy fewer, KV is causal)
// The tensors' bases and per-position bytes (up to 80 layers x 5 kinds) live in a device table built once per context for its own
// sequence and once for its slots (the caches never move); a slot is reached through its number, since every slot of a tensor is
// rows() * pos_bytes long.
//
// Width, decided per segment: 16 bytes per lane (global_load / store_dwordx4) where the source, the destination and the length are
// all multiples of 16 bytes, else 4 bytes per lane (every segment start and length is a multiple of 4).  With the 256-byte aligned
// allocations of the engine that means
//   f32 rows (256 / 512 B), byte rows (64 / 128 B), tq2 codes (16 / 32 B), tq3 codes at d = 128 (48 B)      always 16 B
//   tq3 codes at d = 64 (24 B)                              16 B when n, n_stride and h * max_seq are even, else 4 B
//   QJL words (12 / 20 B), int8 scales (4 B)                16 B when n, n_stride and h * max_seq are multiples of 4, else 4 B
// so the rows, which are all but a few percent of the bytes, go wide except tq3 / d = 64 at odd sizes; the scales and QJL words
// (4 .. 20 of 132 .. 532 bytes per position) are the ones that fall to the narrow path.
// Plain vector loads and stores, no LDS, no scratch (tests/test_build_props_kv_prefix.py).
#include "engine.h"

#include <algorithm>

using namespace lgh;

namespace lgh {

// one (owned layer, kind) of the table: the tensor (slot 0 of it), the bytes per position, and the sum of the bytes per position of
// the entries before it (times n_kv * n_stride: where its segments start in the packed buffer)
struct KvPrefixSeg {
  uint8_t* base;
  uint32_t pos_bytes;
  uint32_t pb_before;
};

constexpr uint32_t kPrefixThreads = 256, kPrefixUnroll = 4;

// `count` elements of a segment, this lane's share: passes of kPrefixUnroll elements kPrefixThreads apart, all loaded before the first
// is stored (named values, not an array: the compiler moves a conditionally written array of them to LDS); then the last, partial pass
// (pointers into global memory, said so: a tensor's base is loaded from the table, and a pointer that comes out of memory would
// otherwise be a generic one, stored through flat_store)
#define LGH_GLOBAL __attribute__((address_space(1)))
typedef uint32_t PrefixWide __attribute__((ext_vector_type(4)));
template <class T>
__device__ __forceinline__ void prefix_copy_lane(const LGH_GLOBAL T* __restrict__ s, LGH_GLOBAL T* __restrict__ d, uint64_t count, uint64_t first,
                                                 uint64_t step) {
  static_assert(kPrefixUnroll == 4, "four named values per pass");
  constexpr uint64_t W = kPrefixThreads;
  uint64_t i = first;
  for (; i + 3 * W < count; i += step) {
    const T a = s[i], b = s[i + W], c = s[i + 2 * W], e = s[i + 3 * W];
    d[i] = a;
    d[i + W] = b;
    d[i + 2 * W] = c;
    d[i + 3 * W] = e;
  }
  for (uint64_t j = i; j < count && j < i + 3 * W; j += W) d[j] = s[j];   // (a pass behind this one starts past count)
}

template <bool RESTORE>
__global__ __launch_bounds__(kPrefixThreads) void kv_prefix_copy_kernel(const KvPrefixSeg* __restrict__ table, uint8_t* __restrict__ packed,
                                                                        uint32_t slot, uint32_t n_kv, uint32_t max_seq, uint32_t n,
                                                                        uint32_t n_stride) {
  const uint32_t e = blockIdx.x / n_kv, h = blockIdx.x - e * n_kv;
  const KvPrefixSeg s = table[e];
  const uint64_t pb = s.pos_bytes, len = (uint64_t)n * pb;
  uint8_t* const cache = s.base + ((uint64_t)slot * n_kv + h) * max_seq * pb;
  uint8_t* const pk = packed + ((uint64_t)s.pb_before * n_kv + (uint64_t)h * pb) * n_stride;
  const LGH_GLOBAL uint8_t* const src = (const LGH_GLOBAL uint8_t*)(RESTORE ? pk : cache);
  LGH_GLOBAL uint8_t* const dst = (LGH_GLOBAL uint8_t*)(RESTORE ? cache : pk);
  const uint64_t first = (uint64_t)blockIdx.y * (kPrefixThreads * kPrefixUnroll) + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.y * (kPrefixThreads * kPrefixUnroll);
  if ((((uint64_t)(uintptr_t)src | (uint64_t)(uintptr_t)dst | len) & 15u) == 0)
    prefix_copy_lane((const LGH_GLOBAL PrefixWide*)src, (LGH_GLOBAL PrefixWide*)dst, len >> 4, first, step);
  else
    prefix_copy_lane((const LGH_GLOBAL uint32_t*)src, (LGH_GLOBAL uint32_t*)dst, len >> 2, first, step);
}

}  // namespace lgh

// bytes of n_rows packed rows of this context's layers
uint64_t kv_prefix_bytes(const lgh_ctx* c, uint64_t n_rows) {
  const KvLayout& l = c->kvl;
  return (uint64_t)(c->l1 - c->l0) * l.n_kv * n_rows * (2 * (l.row_bytes() + l.scale_bytes()) + l.qjl_bytes());
}

// The device table of the own sequence's tensors (slots = false) or of the slots' (the multi-sequence engine's, slot 0 of each): built
// at the first call that needs it, then kept with the context.  (Not counted in lgh_stats: the accounting stays as it was.)
static int prefix_table(lgh_ctx* c, bool slots, const KvPrefixSeg** out, uint32_t* n_entries) {
  void*& tab = c->prefix_tab[slots ? 1 : 0];
  uint32_t& count = c->prefix_tab_n[slots ? 1 : 0];
  if (!tab) {
    std::vector<KvPrefixSeg> host;
    uint32_t before = 0;
    for (uint32_t li = c->l0; li < c->l1; li++) {
      const KvCache& kv = slots ? c->batch.kv[li] : c->layers[li].kv;
      for (int kind = 0; kind < KV_KINDS; kind++) {
        const uint32_t pb = (uint32_t)c->kvl.pos_bytes(kind);
        if (!pb) continue;
        if (!kv.t[kind]) return fail(c, LGH_OPERATION_FAILED, "a KV cache tensor of the format is missing");
        host.push_back(KvPrefixSeg{(uint8_t*)kv.t[kind], pb, before});
        before += pb;
      }
    }
    void* p = nullptr;
    if (int rc = dev_alloc(c, &p, host.size() * sizeof(KvPrefixSeg))) return rc;
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync(p, host.data(), host.size() * sizeof(KvPrefixSeg), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));   // (host is a local)
    tab = p;
    count = (uint32_t)host.size();
  }
  *out = (const KvPrefixSeg*)tab;
  *n_entries = count;
  return LGH_OK;
}

// rows [0, n_rows) of every tensor of every owned layer of the sequence (slot < 0: the context's own) to (restore: from) a packed
// buffer of n_stride rows, enqueued on the context's stream: one launch
int kv_prefix_copy(lgh_ctx* c, int slot, uint32_t n_rows, uint32_t n_stride, void* packed, bool restore) {
  const KvLayout& l = c->kvl;
  if (n_rows == 0 || n_rows > n_stride || n_rows > l.max_seq || !packed) return fail(c, LGH_INVALID_ARGUMENT, "kv_prefix_copy: bad row count");
  if (slot >= 0 && (uint32_t)slot >= c->batch.max_batch) return fail(c, LGH_INVALID_ARGUMENT, "kv_prefix_copy: no such slot");
  const KvPrefixSeg* table = nullptr;
  uint32_t n_entries = 0;
  if (int rc = prefix_table(c, slot >= 0, &table, &n_entries)) return rc;
  const uint64_t segs = (uint64_t)n_entries * l.n_kv;
  if (segs == 0 || segs > 0x7FFFFFFFull) return fail(c, LGH_UNSUPPORTED, "kv_prefix_copy: segment count");
  // memory-bound: up to ~4096 workgroups, each pass of one moving 256 lanes x 4 x 16 bytes of its segment; the rest is grid-strided
  const uint64_t per_wg = (uint64_t)kPrefixThreads * kPrefixUnroll * 16;
  const uint64_t want = ((uint64_t)n_rows * l.row_bytes() + per_wg - 1) / per_wg;
  const uint64_t cap = std::max<uint64_t>(1, 4096 / segs);
  const dim3 grid((uint32_t)segs, (uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 1), std::min<uint64_t>(cap, 65535)));
  const uint32_t s = slot < 0 ? 0u : (uint32_t)slot;
  if (restore)
    hipLaunchKernelGGL(kv_prefix_copy_kernel<true>, grid, dim3(kPrefixThreads), 0, c->stream, table, (uint8_t*)packed, s, l.n_kv, l.max_seq, n_rows, n_stride);
  else
    hipLaunchKernelGGL(kv_prefix_copy_kernel<false>, grid, dim3(kPrefixThreads), 0, c->stream, table, (uint8_t*)packed, s, l.n_kv, l.max_seq, n_rows, n_stride);
  HIP_TRY(c, LGH_OPERATION_FAILED, hipGetLastError());
  return LGH_OK;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
struct lgh_prefix {
  void* dev = nullptr;      // the packed rows
  uint64_t bytes = 0;
  uint32_t n_rows = 0;
};

namespace {

// the fixed header of an exported prefix; the packed rows follow it
struct PrefixHeader {
  uint32_t magic, version, kv_cache_type, num_kv_heads, head_dim, layer_begin, layer_end, n_rows;
  uint64_t payload_bytes;
};
constexpr uint32_t kPrefixMagic = 0x5850474Cu /* "LGPX" */, kPrefixVersion = 1;

bool prefix_live(const lgh_ctx* c, const lgh_prefix* p) {   // by address only: p may be freed or another context's
  return p && std::find(c->prefixes.begin(), c->prefixes.end(), p) != c->prefixes.end();
}

// the position of the sequence; false: no such sequence
bool seq_pos(const lgh_ctx* c, int slot, size_t* pos) {
  if (slot == -1) { *pos = c->pos; return true; }
  if (slot < 0 || !c->batch.ready || (uint32_t)slot >= c->batch.max_batch) return false;
  *pos = c->batch.pos[(size_t)slot];
  return true;
}

int prefix_new(lgh_ctx* c, uint32_t n_rows, lgh_prefix** out) {   // one device allocation, on the context's live list
  lgh_prefix* p = new lgh_prefix();
  p->n_rows = n_rows;
  p->bytes = kv_prefix_bytes(c, n_rows);
  const hipError_t e = hipMalloc(&p->dev, p->bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    delete p;
    return fail(c, LGH_ALLOCATION_FAILED, std::string("hipMalloc(") + std::to_string(kv_prefix_bytes(c, n_rows)) + "): " + hipGetErrorString(e));
  }
  c->prefixes.push_back(p);
  *out = p;
  return LGH_OK;
}

void prefix_drop(lgh_ctx* c, lgh_prefix* p) {
  c->prefixes.erase(std::find(c->prefixes.begin(), c->prefixes.end(), p));
  (void)hipFree(p->dev);
  delete p;
}

}  // namespace

void kv_prefix_release(lgh_ctx* c) {   // lgh_destroy, behind its synchronisation
  while (!c->prefixes.empty()) prefix_drop(c, c->prefixes.back());
}

extern "C" {

int lgh_prefix_save(lgh_ctx* c, int slot, size_t n_rows, lgh_prefix** out) {   // PrefixSharing::save_prefix (cache.rs:313-326)
  int rc = check_ready(c);
  if (rc) return rc;
  if (!out) return fail(c, LGH_INVALID_ARGUMENT, "out is NULL");
  size_t pos = 0;
  if (!seq_pos(c, slot, &pos)) return fail(c, LGH_INVALID_ARGUMENT, "no such slot (lgh_batch_create first)");
  if (n_rows == 0) n_rows = pos;
  if (n_rows == 0) return fail(c, LGH_INVALID_ARGUMENT, "nothing to save: the sequence is at position 0");
  if (n_rows > pos) return fail(c, LGH_INVALID_ARGUMENT, "n_rows exceeds the sequence's position");
  lgh_prefix* p = nullptr;
  if ((rc = prefix_new(c, (uint32_t)n_rows, &p))) return rc;
  if ((rc = kv_prefix_copy(c, slot, p->n_rows, p->n_rows, p->dev, false))) { prefix_drop(c, p); return rc; }
  *out = p;
  return LGH_OK;
}

int lgh_prefix_restore(lgh_ctx* c, const lgh_prefix* p, int slot, size_t n_rows) {   // PrefixSharing::try_restore (cache.rs:269-310)
  int rc = check_ready(c);
  if (rc) return rc;
  if (!prefix_live(c, p)) return fail(c, LGH_INVALID_ARGUMENT, "not a live prefix of this context");
  size_t pos = 0;
  if (!seq_pos(c, slot, &pos)) return fail(c, LGH_INVALID_ARGUMENT, "no such slot (lgh_batch_create first)");
  if (n_rows == 0) n_rows = p->n_rows;
  if (n_rows > p->n_rows) return fail(c, LGH_INVALID_ARGUMENT, "n_rows exceeds the prefix's rows");
  if ((rc = kv_prefix_copy(c, slot, (uint32_t)n_rows, p->n_rows, p->dev, true))) return rc;
  if (slot < 0) {   // as prefill_own leaves them
    c->pos = n_rows;
    HIP_TRY(c, LGH_OPERATION_FAILED, hipMemsetD32Async((hipDeviceptr_t)(c->state + ST_NEXT), (int)c->pos, 1, c->stream));
  } else {
    c->batch.pos[(size_t)slot] = n_rows;
  }
  return LGH_OK;
}

int lgh_prefix_free(lgh_ctx* c, lgh_prefix* p) {   // PromptCache::remove_prefix (cache.rs:191-195)
  int rc = check_ready(c);
  if (rc) return rc;
  if (!prefix_live(c, p)) return fail(c, LGH_INVALID_ARGUMENT, "not a live prefix of this context");
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));   // (a save or restore of it may still be in flight)
  prefix_drop(c, p);
  return LGH_OK;
}

int lgh_prefix_get_info(lgh_ctx* c, const lgh_prefix* p, lgh_prefix_info* info) {   // CachedPrefix::seq_len / memory_size (cache.rs:38, 60-64)
  int rc = check_ready(c);
  if (rc) return rc;
  if (!info) return fail(c, LGH_INVALID_ARGUMENT, "info is NULL");
  if (!prefix_live(c, p)) return fail(c, LGH_INVALID_ARGUMENT, "not a live prefix of this context");
  *info = lgh_prefix_info{(uint32_t)sizeof(lgh_prefix_info), c->kvl.type, p->n_rows, c->l0, c->l1, p->bytes};
  return LGH_OK;
}

uint64_t lgh_prefix_total_bytes(lgh_ctx* c) {   // PromptCacheStats::memory_used (cache.rs:203-210), device bytes only
  uint64_t n = 0;
  if (c)
    for (const lgh_prefix* p : c->prefixes) n += p->bytes;
  return n;
}

int lgh_prefix_export(lgh_ctx* c, const lgh_prefix* p, void* dst, size_t dst_bytes, size_t* needed) {   // CachedPrefix as bytes (cache.rs:28-43)
  int rc = check_ready(c);
  if (rc) return rc;
  if (!prefix_live(c, p)) return fail(c, LGH_INVALID_ARGUMENT, "not a live prefix of this context");
  const size_t total = sizeof(PrefixHeader) + (size_t)p->bytes;
  if (needed) *needed = total;
  if (!dst) return needed ? LGH_OK : fail(c, LGH_INVALID_ARGUMENT, "dst and needed are both NULL");   // (a size query)
  if (dst_bytes < total) return fail(c, LGH_INVALID_ARGUMENT, "dst holds fewer bytes than the prefix needs");
  const PrefixHeader h{kPrefixMagic, kPrefixVersion, c->kvl.type, c->kvl.n_kv, c->kvl.d, c->l0, c->l1, p->n_rows, p->bytes};
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  std::memcpy(dst, &h, sizeof(h));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipMemcpyAsync((uint8_t*)dst + sizeof(h), p->dev, p->bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, LGH_OPERATION_FAILED, hipStreamSynchronize(c->stream));
  return LGH_OK;
}

int lgh_prefix_import(lgh_ctx* c, const void* src, size_t bytes, lgh_prefix** out) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!src || !out) return fail(c, LGH_INVALID_ARGUMENT, "src / out is NULL");
  PrefixHeader h;
  if (bytes < sizeof(h)) return fail(c, LGH_INVALID_ARGUMENT, "shorter than a prefix header");
  std::memcpy(&h, src, sizeof(h));
  if (h.magic != kPrefixMagic || h.version != kPrefixVersion) return fail(c, LGH_INVALID_ARGUMENT, "not an exported prefix of this version");
  if (h.kv_cache_type != c->kvl.type || h.num_kv_heads != c->kvl.n_kv || h.head_dim != c->kvl.d || h.layer_begin != c->l0 || h.layer_end != c->l1)
    return fail(c, LGH_INVALID_ARGUMENT, "the prefix was saved with another cache format, shape or layer range");
  if (h.n_rows == 0 || h.n_rows > c->kvl.max_seq) return fail(c, LGH_INVALID_ARGUMENT, "the prefix's rows do not fit this context");
  if (h.payload_bytes != kv_prefix_bytes(c, h.n_rows) || bytes != sizeof(h) + h.payload_bytes)
    return fail(c, LGH_INVALID_ARGUMENT, "the prefix's size does not match its header");
  lgh_prefix* p = nullptr;
  if ((rc = prefix_new(c, h.n_rows, &p))) return rc;
  if (hipMemcpyAsync(p->dev, (const uint8_t*)src + sizeof(h), p->bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    prefix_drop(c, p);
    return fail(c, LGH_OPERATION_FAILED, "copying the prefix to the device");
  }
  *out = p;
  return LGH_OK;
}

}  // extern "C"
