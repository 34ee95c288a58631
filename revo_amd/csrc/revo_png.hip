// revo_png.hip -- PNG decoding on the device (the cv::imread of iowrapperRGBD.cpp:257-333, for the multi-stream front-end).
//   * Host: the chunk list is parsed and checked (signature, CRCs, IHDR); the IDAT payloads of a batch are packed behind their
//     job descriptors in one page-locked slab and go to the device in ONE copy.
//   * k_png_inflate: one wave64 per image runs the inflate core of revo_inflate.h (zlib header, stored / fixed / dynamic
//     blocks, Adler-32) with its 32 KiB window, input window and code tables in LDS; the filtered scanlines go to a scratch slab.
//   * k_png_unfilter: one workgroup per image undoes the per-row filters (None / Sub / Up / Average / Paeth: a row depends on
//     the one before; Sub, Average and Paeth are serial along the row with stride bpp, so bpp lanes run those chains) and
//     writes the caller's layout (BGR8 or native u16).
//   * A corrupt image sets its own status word and nothing else: every read is bounded by its compressed length, every write
//     by its raw size and destination rows, every loop by those sizes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "revo_internal.h"
#include "revo_inflate.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- host parse --
uint32_t crc_table[256];
bool crc_ready = false;
uint32_t crc32(const uint8_t* p, size_t n) {
  if (!crc_ready) {  // (idempotent: a race writes the same values)
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
      crc_table[i] = c;
    }
    crc_ready = true;
  }
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) c = crc_table[(c ^ p[i]) & 255] ^ (c >> 8);
  return c ^ 0xffffffffu;
}
uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

struct Span { size_t off, len; };

// Parses and checks the chunk list; fills *info and (if spans) the IDAT payload spans.  REVO_ERR_CORRUPT with a message for a
// malformed file, REVO_ERR_UNSUPPORTED (info filled) for a valid file the device decoder does not handle.
int parse(const uint8_t* png, size_t len, revo_png_info* info, std::vector<Span>* spans, std::string* why) {
  static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  memset(info, 0, sizeof(*info));
  if (spans) spans->clear();
  auto corrupt = [&](const char* m) { *why = m; return REVO_ERR_CORRUPT; };
  if (!png || len < 8 || memcmp(png, sig, 8) != 0) return corrupt("not a PNG signature");
  size_t pos = 8;
  bool have_ihdr = false, have_iend = false, unknown_critical = false;
  uint64_t idat = 0;
  while (pos < len) {
    if (len - pos < 12) return corrupt("truncated chunk");
    const uint32_t n = be32(png + pos);
    if (n > 0x7fffffffu || (uint64_t)n > len - pos - 12) return corrupt("chunk length out of range");
    const uint8_t* type = png + pos + 4;
    const uint8_t* data = png + pos + 8;
    if (crc32(type, (size_t)n + 4) != be32(data + n)) return corrupt("chunk CRC mismatch");
    if (!have_ihdr && memcmp(type, "IHDR", 4) != 0) return corrupt("the first chunk is not IHDR");
    if (memcmp(type, "IHDR", 4) == 0) {
      if (have_ihdr || n != 13) return corrupt("bad IHDR");
      have_ihdr = true;
      info->width = (int32_t)be32(data);
      info->height = (int32_t)be32(data + 4);
      info->bit_depth = data[8];
      info->color_type = data[9];
      info->interlace = data[12];
      if (be32(data) == 0 || be32(data + 4) == 0 || be32(data) > 0x7fffffffu || be32(data + 4) > 0x7fffffffu)
        return corrupt("zero or out-of-range image size");
      if (data[10] != 0 || data[11] != 0 || data[12] > 1) return corrupt("bad compression, filter or interlace method");
      const int d = data[8], ct = data[9];
      const bool ok = (ct == 0 && (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)) || (ct == 3 && d <= 8 && (d & (d - 1)) == 0) ||
                      ((ct == 2 || ct == 4 || ct == 6) && (d == 8 || d == 16));
      if (!ok) return corrupt("bad bit depth / colour type combination");
    } else if (memcmp(type, "IDAT", 4) == 0) {
      idat += n;
      if (spans) spans->push_back(Span{pos + 8, n});
    } else if (memcmp(type, "IEND", 4) == 0) {
      have_iend = true;
      break;
    } else if (!(type[0] & 0x20) && memcmp(type, "PLTE", 4) != 0) {
      unknown_critical = true;
    }
    pos += (size_t)n + 12;
  }
  if (!have_ihdr) return corrupt("no IHDR");
  if (!have_iend) return corrupt("no IEND");
  if (idat == 0) return corrupt("no image data");
  const uint64_t ch = info->color_type == 0 ? 1 : info->color_type == 2 ? 3 : info->color_type == 3 ? 1 : info->color_type == 4 ? 2 : 4;
  const uint64_t rowbits = (uint64_t)info->width * ch * (uint64_t)info->bit_depth;
  info->idat_bytes = idat;
  info->raw_bytes = (uint64_t)info->height * (1 + (rowbits + 7) / 8);
  if (info->interlace) { *why = "interlaced (Adam7)"; return REVO_ERR_UNSUPPORTED; }
  if (info->color_type == 3) { *why = "palette"; return REVO_ERR_UNSUPPORTED; }
  if (info->bit_depth < 8) { *why = "bit depth below 8"; return REVO_ERR_UNSUPPORTED; }
  if (info->bit_depth == 16 && info->color_type != 0) { *why = "16-bit colour"; return REVO_ERR_UNSUPPORTED; }
  if (unknown_critical) { *why = "unknown critical chunk"; return REVO_ERR_UNSUPPORTED; }
  return REVO_OK;
}

// ------------------------------------------------------------------------------------------------------------------- device --
constexpr int MAX_ROW = 8192;  // bytes of one unfiltered row the unfilter kernel stages (2048 RGBA pixels)

struct PngDesc {
  uint64_t comp_off, comp_len;  // in the device slab
  uint64_t raw_off, raw_bytes;  // in the scratch slab
  uint8_t* dst;
  uint64_t dst_stride;
  int32_t width, height, color_type, bit_depth, format, idx;
};

struct WavePar {
  __device__ int lane() const { return (int)threadIdx.x; }
  __device__ int nlanes() const { return 64; }
  __device__ void sync() const { __syncthreads(); }
  __device__ uint32_t sum(uint32_t v) const {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  }
};

__global__ void __launch_bounds__(64) k_png_inflate(const PngDesc* __restrict__ descs, const uint8_t* __restrict__ slab,
                                                    uint8_t* __restrict__ raw, int32_t* __restrict__ status) {
  __shared__ uint8_t ring[rinf::RING];
  __shared__ uint8_t win[rinf::IN_WIN];
  __shared__ uint8_t lens[rinf::MAX_LENS];
  __shared__ uint16_t tab[2 * (16 + 16 + rinf::FAST) + rinf::MAX_LIT + rinf::MAX_DIST];
  const PngDesc d = descs[blockIdx.x];
  rinf::Mem m;
  uint16_t* q = tab;
  m.ring = ring; m.win = win; m.lens = lens;
  m.lcount = q; q += 16; m.loffs = q; q += 16; m.lsym = q; q += rinf::MAX_LIT; m.lfast = q; q += rinf::FAST;
  m.dcount = q; q += 16; m.doffs = q; q += 16; m.dsym = q; q += rinf::MAX_DIST; m.dfast = q;
  rinf::Inflater<WavePar> inf(WavePar(), m, slab + d.comp_off, d.comp_len, raw + d.raw_off, d.raw_bytes);
  const int e = inf.run();
  if (threadIdx.x == 0) status[d.idx] = e == rinf::OK ? REVO_OK : REVO_ERR_CORRUPT;
}

__device__ __forceinline__ uint8_t paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (uint8_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

__global__ void __launch_bounds__(256) k_png_unfilter(const PngDesc* __restrict__ descs, uint8_t* __restrict__ raw,
                                                      int32_t* __restrict__ status) {
  __shared__ uint8_t rows[2][MAX_ROW];
  const PngDesc d = descs[blockIdx.x];
  if (status[d.idx] != REVO_OK) return;  // (uniform: the inflate of this image failed)
  const int t = (int)threadIdx.x, nt = (int)blockDim.x;
  const int ch = d.color_type == 0 ? 1 : d.color_type == 2 ? 3 : d.color_type == 4 ? 2 : 4;
  const int bpp = ch * (d.bit_depth / 8);
  const int rb = d.width * bpp, w = d.width;
  uint8_t* prev = rows[0];
  uint8_t* cur = rows[1];
  for (int k = t; k < rb; k += nt) prev[k] = 0;
  const uint8_t* src = raw + d.raw_off;
  bool ok = true;
  for (int y = 0; y < d.height; ++y) {
    const uint8_t* s = src + (size_t)y * (size_t)(rb + 1);
    const int ft = s[0];
    if (ft > 4) { ok = false; break; }
    for (int k = t; k < rb; k += nt) cur[k] = s[1 + k];
    __syncthreads();
    if (ft == 2) {
      for (int k = t; k < rb; k += nt) cur[k] = (uint8_t)(cur[k] + prev[k]);
    } else if (ft != 0 && t < bpp) {  // one serial chain per byte of a pixel
      int a = 0, c = 0;
      for (int x = t; x < rb; x += bpp) {
        const int b = prev[x];
        const int pred = ft == 1 ? a : ft == 3 ? ((a + b) >> 1) : paeth(a, b, c);
        const uint8_t v = (uint8_t)(cur[x] + pred);
        cur[x] = v;
        a = v;
        c = b;
      }
    }
    __syncthreads();
    uint8_t* o = d.dst + (size_t)y * d.dst_stride;
    if (d.format == REVO_PNG_BGR8) {
      for (int x = t; x < w; x += nt) {
        uint8_t r, g, b;
        if (ch >= 3) { r = cur[x * ch]; g = cur[x * ch + 1]; b = cur[x * ch + 2]; }
        else { r = g = b = cur[x * ch]; }
        o[3 * x] = b; o[3 * x + 1] = g; o[3 * x + 2] = r;
      }
    } else {
      uint16_t* o16 = (uint16_t*)o;
      if (d.bit_depth == 16) for (int x = t; x < w; x += nt) o16[x] = (uint16_t)((cur[2 * x] << 8) | cur[2 * x + 1]);
      else for (int x = t; x < w; x += nt) o16[x] = cur[x];
    }
    uint8_t* tmp = prev; prev = cur; cur = tmp;
  }
  __syncthreads();
  if (!ok && t == 0) status[d.idx] = REVO_ERR_CORRUPT;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------- C ABI --
extern "C" int revo_png_probe(const uint8_t* png, size_t len, revo_png_info* out) {
  if (!out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  std::string why;
  const int rc = parse(png, len, out, nullptr, &why);
  if (rc) return fail(rc, why);
  return REVO_OK;
}

namespace {
constexpr int SLOTS = 2;  // tickets that may be outstanding at once
struct Slot {
  uint64_t ticket = 0;
  bool busy = false;
  int n = 0;
  std::vector<int32_t> host_status;  // codes found on the host (REVO_OK: decided on the device)
  int32_t* h_status = nullptr;       // page-locked, filled by the D2H copy
  int32_t* d_status = nullptr;
  hipEvent_t done = nullptr;
};
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
}  // namespace

struct revo_png_decoder {
  revo_ctx* ctx = nullptr;
  int device = 0, max_images = 0;
  size_t max_comp = 0, max_raw = 0, slab_bytes = 0;
  uint8_t* h_slab = nullptr;  // page-locked: descriptors, then the packed IDAT payloads
  uint8_t* d_slab = nullptr;
  uint8_t* d_raw = nullptr;   // filtered scanlines, max_raw per image
  hipEvent_t ev_h2d = nullptr, ev_done = nullptr;
  bool has_h2d = false, has_done = false;
  uint64_t next_ticket = 1;
  Slot slot[SLOTS];
};

extern "C" void revo_png_decoder_destroy(revo_png_decoder* d) {
  if (!d) return;
  hipSetDevice(d->device);
  for (Slot& s : d->slot) {
    if (s.done) { hipEventSynchronize(s.done); hipEventDestroy(s.done); }
    hipHostFree(s.h_status);
    hipFree(s.d_status);
  }
  if (d->ev_h2d) hipEventDestroy(d->ev_h2d);
  if (d->ev_done) { hipEventSynchronize(d->ev_done); hipEventDestroy(d->ev_done); }
  hipHostFree(d->h_slab);
  hipFree(d->d_slab);
  hipFree(d->d_raw);
  (void)hipGetLastError();
  if (d->ctx) revo_ctx_release_(d->ctx);
  delete d;
}

extern "C" int revo_png_decoder_create(revo_ctx* ctx, int max_images, size_t max_compressed_bytes, size_t max_raw_bytes_per_image,
                                       revo_png_decoder** out) {
  if (!out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (max_images < 1 || max_images > (1 << 20) || max_compressed_bytes < 1 || max_raw_bytes_per_image < 1)
    return fail(REVO_ERR_INVALID_ARG, "max_images, max_compressed_bytes and max_raw_bytes_per_image must be positive");
  revo_png_decoder* d = new revo_png_decoder();
  struct Guard { revo_png_decoder* d; ~Guard() { if (d) revo_png_decoder_destroy(d); } } guard{d};
  if (ctx) {
    d->ctx = ctx;
    revo_ctx_retain_(ctx);
    d->device = revo_ctx_device_(ctx);
  } else {
    HIPCHECK(hipGetDevice(&d->device));
  }
  HIPCHECK(hipSetDevice(d->device));
  d->max_images = max_images;
  d->max_comp = max_compressed_bytes;
  d->max_raw = align_up(max_raw_bytes_per_image, 256);
  d->slab_bytes = align_up(sizeof(PngDesc) * (size_t)max_images, 256) + max_compressed_bytes;
  HIPCHECK(hipHostMalloc((void**)&d->h_slab, d->slab_bytes));
  HIPCHECK(hipMalloc((void**)&d->d_slab, d->slab_bytes));
  HIPCHECK(hipMalloc((void**)&d->d_raw, d->max_raw * (size_t)max_images));
  HIPCHECK(hipEventCreateWithFlags(&d->ev_h2d, hipEventDisableTiming));
  HIPCHECK(hipEventCreateWithFlags(&d->ev_done, hipEventDisableTiming));
  for (Slot& s : d->slot) {
    HIPCHECK(hipHostMalloc((void**)&s.h_status, sizeof(int32_t) * max_images));
    HIPCHECK(hipMalloc((void**)&s.d_status, sizeof(int32_t) * max_images));
    HIPCHECK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    s.host_status.assign(max_images, 0);
  }
  guard.d = nullptr;
  *out = d;
  return REVO_OK;
}

extern "C" int revo_png_decode_submit(revo_png_decoder* d, int n, const revo_png_job* jobs, void* stream, uint64_t* ticket) {
  if (!d || !ticket || n < 0 || (n > 0 && !jobs)) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  if (n > d->max_images) return fail(REVO_ERR_CAPACITY, "more images than the decoder was created for");
  Slot* sl = nullptr;
  for (Slot& s : d->slot)
    if (!s.busy) { sl = &s; break; }
  if (!sl) return fail(REVO_ERR_CAPACITY, "two decodes are outstanding: revo_png_decode_wait for one first");
  for (int i = 0; i < n; ++i) {
    const revo_png_job& j = jobs[i];
    if (j.format != REVO_PNG_BGR8 && j.format != REVO_PNG_U16) return fail(REVO_ERR_INVALID_ARG, "unknown output format");
    if (!j.d_dst || j.width < 1 || j.height < 1) return fail(REVO_ERR_INVALID_ARG, "null destination or bad size");
    const size_t px = j.format == REVO_PNG_BGR8 ? 3 : 2;
    if (j.dst_stride < (size_t)j.width * px || (j.format == REVO_PNG_U16 && (((uintptr_t)j.d_dst | j.dst_stride) & 1)))
      return fail(REVO_ERR_INVALID_ARG, "destination stride smaller than a row, or a u16 destination not 2-byte aligned");
  }
  HIPCHECK(hipSetDevice(d->device));
  hipStream_t s = (hipStream_t)stream;
  // the previous batch's copy has read the page-locked slab
  if (d->has_h2d) HIPCHECK(hipEventSynchronize(d->ev_h2d));
  // host side: parse every file, keep the ones the device decodes, pack their IDAT payloads
  const size_t desc_bytes = align_up(sizeof(PngDesc) * (size_t)n, 256);
  PngDesc* descs = (PngDesc*)d->h_slab;
  uint8_t* data = d->h_slab + desc_bytes;
  const size_t data_cap = d->slab_bytes - desc_bytes;
  std::vector<Span> spans;
  size_t used = 0;
  int nl = 0;
  revo_png_info info;
  std::string why;
  for (int i = 0; i < n; ++i) {
    const revo_png_job& j = jobs[i];
    int st = parse(j.png, j.len, &info, &spans, &why);
    if (st == REVO_OK && (info.width != j.width || info.height != j.height)) st = REVO_ERR_INVALID_ARG;
    if (st == REVO_OK) {
      const int ct = info.color_type, bd = info.bit_depth;
      const bool fits = j.format == REVO_PNG_BGR8 ? bd == 8 : ct == 0;
      const uint64_t rb = info.raw_bytes / (uint64_t)info.height - 1;
      if (!fits || rb > (uint64_t)MAX_ROW) st = REVO_ERR_UNSUPPORTED;
      else if (info.raw_bytes > d->max_raw) return fail(REVO_ERR_CAPACITY, "an image is larger than max_raw_bytes_per_image");
    }
    sl->host_status[i] = st;
    if (st != REVO_OK) continue;
    if (info.idat_bytes > data_cap - used) return fail(REVO_ERR_CAPACITY, "the batch's image data exceed max_compressed_bytes");
    PngDesc& pd = descs[nl];
    pd.comp_off = desc_bytes + used;
    pd.comp_len = info.idat_bytes;
    for (const Span& sp : spans) { memcpy(data + used, j.png + sp.off, sp.len); used += sp.len; }
    pd.raw_off = (uint64_t)nl * d->max_raw;
    pd.raw_bytes = info.raw_bytes;
    pd.dst = (uint8_t*)j.d_dst;
    pd.dst_stride = j.dst_stride;
    pd.width = info.width; pd.height = info.height; pd.color_type = info.color_type; pd.bit_depth = info.bit_depth;
    pd.format = j.format;
    pd.idx = i;
    ++nl;
  }
  // the previous batch's kernels are done with the device slab, the scratch and (same slot) the status words
  if (d->has_done) HIPCHECK(hipStreamWaitEvent(s, d->ev_done, 0));
  if (nl > 0) {
    HIPCHECK(hipMemcpyAsync(d->d_slab, d->h_slab, desc_bytes + used, hipMemcpyHostToDevice, s));
    HIPCHECK(hipEventRecord(d->ev_h2d, s));
    d->has_h2d = true;
    const PngDesc* dd = (const PngDesc*)d->d_slab;
    hipLaunchKernelGGL(k_png_inflate, dim3(nl), dim3(64), 0, s, dd, d->d_slab, d->d_raw, sl->d_status);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_png_unfilter, dim3(nl), dim3(256), 0, s, dd, d->d_raw, sl->d_status);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(sl->h_status, sl->d_status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  }
  HIPCHECK(hipEventRecord(d->ev_done, s));
  d->has_done = true;
  HIPCHECK(hipEventRecord(sl->done, s));
  sl->busy = true;
  sl->n = n;
  sl->ticket = d->next_ticket++;
  *ticket = sl->ticket;
  return REVO_OK;
}

extern "C" int revo_png_decode_wait(revo_png_decoder* d, uint64_t ticket, int32_t* status) {
  if (!d) return fail(REVO_ERR_INVALID_ARG, "null decoder");
  Slot* sl = nullptr;
  for (Slot& s : d->slot)
    if (s.busy && s.ticket == ticket) sl = &s;
  if (!sl) return fail(REVO_ERR_INVALID_ARG, "unknown or already waited ticket");
  HIPCHECK(hipSetDevice(d->device));
  HIPCHECK(hipEventSynchronize(sl->done));
  sl->busy = false;
  if (status)
    for (int i = 0; i < sl->n; ++i) status[i] = sl->host_status[i] != REVO_OK ? sl->host_status[i] : sl->h_status[i];
  return REVO_OK;
}
