// revo_inflate.h -- the serial core of zlib inflate (RFC 1950 / 1951), written once for the device decoder (revo_png.hip, one
// wave64 per image) and for a host build that is checked against zlib on a machine without a GPU (tests/cpp/inflate_harness.cpp).
//
// Every lane of the wave runs the same bit reader, table builder and symbol loop on the same values (wave-uniform control, no
// divergence); the lanes split only the data-parallel parts: table fills, match copies, input staging and output flushes.  The
// policy P says how: P::lane(), P::nlanes(), P::sync() (a barrier between lanes) and P::sum() (a sum over the lanes).  The host
// policy is one lane.
//
// Storage (the caller's; LDS on the device):
//   - a 32 KiB ring holding the last 32 KiB of output (the longest distance), so a match never re-reads global memory;
//   - a window of IN_WIN staged input bytes, refilled by the whole wave;
//   - code counts, symbols and a 2^FAST_BITS-entry first-level table for each of the two codes in use.
// Output leaves the ring in FLUSH-byte chunks, and the Adler-32 of the inflated bytes is accumulated as it leaves.
//
// Untrusted input: every input read is bounded by in_len, every output write by out_len, and every loop by those sizes; any
// fault ends the run with an error code (nothing is read or written out of range).
#ifndef REVO_INFLATE_H
#define REVO_INFLATE_H

#include <stddef.h>
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define RI_HD __host__ __device__ inline

namespace rinf {

enum {
  OK = 0,
  E_HEADER = 1,     // bad zlib header (method, window, check bits)
  E_FDICT = 2,      // preset dictionary (PNG forbids it)
  E_BTYPE = 3,      // block type 3
  E_STORED = 4,     // stored block LEN / NLEN mismatch
  E_CODES = 5,      // invalid code-length set (over-subscribed, incomplete, bad repeat, no end-of-block code)
  E_SYMBOL = 6,     // a code that is not in the table, or literal/length 286-287, distance 30-31
  E_DIST = 7,       // distance reaching before the start of the output
  E_OVERRUN = 8,    // more output than expected
  E_UNDERRUN = 9,   // less output than expected
  E_TRUNCATED = 10, // the input ends inside the stream
  E_ADLER = 11,     // Adler-32 mismatch
  E_BUDGET = 12     // iteration bound hit (cannot happen on a well-formed stream)
};

constexpr int RING = 32768, RING_MASK = RING - 1;
constexpr int IN_WIN = 2048;
constexpr int FLUSH = 4096;  // <= 4096 keeps the per-flush Adler sums in 32 bits
constexpr int FAST_BITS = 9, FAST = 1 << FAST_BITS;
constexpr int MAX_LIT = 288, MAX_DIST = 32, MAX_LENS = 320;

struct Mem {
  uint8_t* ring;                        // RING
  uint8_t* win;                         // IN_WIN
  uint8_t* lens;                        // MAX_LENS
  uint16_t *lcount, *loffs, *lsym, *lfast;  // 16, 16, MAX_LIT, FAST
  uint16_t *dcount, *doffs, *dsym, *dfast;  // 16, 16, MAX_DIST, FAST
};

struct HostPar {
  RI_HD int lane() const { return 0; }
  RI_HD int nlanes() const { return 1; }
  RI_HD void sync() const {}
  RI_HD uint32_t sum(uint32_t v) const { return v; }
};

template <class P>
struct Inflater {
  P par;
  Mem m;
  const uint8_t* in;
  size_t in_len;
  uint8_t* out;
  size_t out_len;
  // bit reader: bb holds bc valid bits, LSB first; ip = next input byte not yet in bb; the window holds in[wbase, wbase + IN_WIN)
  uint64_t bb = 0;
  int bc = 0;
  size_t ip = 0, wbase = 0;
  bool staged = false;
  // output: p bytes produced, the first `flushed` of them written to out; Adler-32 of the flushed bytes
  size_t p = 0, flushed = 0;
  uint32_t ad_a = 1, ad_b = 0;
  int err = OK;

  RI_HD Inflater(P par_, Mem m_, const uint8_t* in_, size_t in_len_, uint8_t* out_, size_t out_len_)
      : par(par_), m(m_), in(in_), in_len(in_len_), out(out_), out_len(out_len_) {}

  // ---- input ----
  RI_HD void stage(size_t at) {  // the whole wave copies in[at, at + IN_WIN) into the window
    par.sync();
    for (size_t k = par.lane(); k < (size_t)IN_WIN && at + k < in_len; k += par.nlanes()) m.win[k] = in[at + k];
    wbase = at;
    staged = true;
    par.sync();
  }
  RI_HD void refill() {
    while (bc <= 56 && ip < in_len) {
      if (!staged || ip < wbase || ip - wbase >= (size_t)IN_WIN) stage(ip);
      bb |= (uint64_t)m.win[ip - wbase] << bc;
      ++ip;
      bc += 8;
    }
  }
  RI_HD uint32_t bits(int n) {  // n <= 32; 0 and err = E_TRUNCATED past the end of the input
    if (bc < n) refill();
    if (bc < n) { err = E_TRUNCATED; return 0; }
    const uint32_t v = (uint32_t)(bb & ((1ull << n) - 1));
    bb >>= n;
    bc -= n;
    return v;
  }

  // ---- Huffman codes (canonical, RFC 1951 3.2.2) ----
  // Canonical decode of the code whose bits (LSB = first bit) are in `v`, at most `maxlen` bits: symbol | len << 9, 0 if none.
  RI_HD static uint32_t walk(const uint16_t* count, const uint16_t* sym, uint64_t v, int maxlen) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= maxlen; ++len) {
      code |= (int)((v >> (len - 1)) & 1);
      const int c = count[len];
      if (code - first < c) return (uint32_t)sym[index + code - first] | ((uint32_t)len << 9);
      index += c;
      first += c;
      first <<= 1;
      code <<= 1;
    }
    return 0;
  }
  // Builds count / symbols / first-level table from n code lengths; codes_table: the code-length code (no incomplete set).
  RI_HD bool build(const uint8_t* lens, int n, uint16_t* count, uint16_t* offs, uint16_t* sym, uint16_t* fast, bool codes_table) {
    par.sync();
    if (par.lane() == 0) {
      for (int l = 0; l < 16; ++l) count[l] = 0;
      for (int s = 0; s < n; ++s) count[lens[s]]++;
      count[0] = 0;
      offs[1] = 0;
      for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + count[l];
      for (int s = 0; s < n; ++s)
        if (lens[s]) sym[offs[lens[s]]++] = (uint16_t)s;
    }
    par.sync();
    int left = 1, total = 0;
    for (int l = 1; l < 16; ++l) {
      left <<= 1;
      left -= count[l];
      total += count[l];
      if (left < 0) { err = E_CODES; return false; }
    }
    // zlib's rule: an incomplete set is allowed only for a single code of length 1 of a literal/length or distance code;
    // an empty set is accepted (any use of it is an invalid symbol)
    if (total > 0 && left > 0 && (codes_table || !(total == 1 && count[1] == 1))) { err = E_CODES; return false; }
    for (int e = par.lane(); e < FAST; e += par.nlanes()) {
      const uint32_t w = walk(count, sym, (uint64_t)e, FAST_BITS);
      fast[e] = (uint16_t)w;
    }
    par.sync();
    return true;
  }
  RI_HD int decode(const uint16_t* count, const uint16_t* sym, const uint16_t* fast) {
    if (bc < 15) refill();
    uint32_t e = fast[bb & (FAST - 1)];
    if (!e) e = walk(count, sym, bb, 15);
    const int len = (int)(e >> 9);
    if (!e) { err = bc < 15 ? E_TRUNCATED : E_SYMBOL; return -1; }
    if (len > bc) { err = E_TRUNCATED; return -1; }
    bb >>= len;
    bc -= len;
    return (int)(e & 511);
  }

  // ---- output ----
  RI_HD void flush(size_t n) {  // ring[flushed, flushed + n) -> out, Adler-32 over it (n <= FLUSH)
    uint32_t s1 = 0, s2 = 0;
    for (size_t k = par.lane(); k < n; k += par.nlanes()) {
      const uint8_t b = m.ring[(flushed + k) & RING_MASK];
      out[flushed + k] = b;
      s1 += b;
      s2 += (uint32_t)(n - k) * b;
    }
    s1 = par.sum(s1);
    s2 = par.sum(s2);
    ad_b = (uint32_t)(((uint64_t)ad_b + (uint64_t)n * ad_a + s2) % 65521u);
    ad_a = (uint32_t)(((uint64_t)ad_a + s1) % 65521u);
    flushed += n;
    par.sync();
  }
  RI_HD void maybe_flush() {
    if (p - flushed >= (size_t)FLUSH) flush(FLUSH);
  }
  RI_HD void literal(uint32_t b) {
    if (p >= out_len) { err = E_OVERRUN; return; }
    m.ring[p & RING_MASK] = (uint8_t)b;  // (every lane writes the same byte)
    ++p;
    maybe_flush();
  }
  RI_HD void match(uint32_t len, uint32_t dist) {
    if (dist > p) { err = E_DIST; return; }
    if (len > out_len - p) { err = E_OVERRUN; return; }
    // out[p + i] = out[p - d + (i mod d)]: every source byte precedes the match, so the lanes copy independently
    for (uint32_t i = par.lane(); i < len; i += par.nlanes())
      m.ring[(p + i) & RING_MASK] = m.ring[(p - dist + (i % dist)) & RING_MASK];
    par.sync();
    p += len;
    maybe_flush();
  }

  // ---- blocks ----
  RI_HD void stored(size_t& budget) {
    bits(bc & 7);
    const uint32_t len = bits(16), nlen = bits(16);
    if (err) return;
    if ((len ^ 0xffffu) != nlen) { err = E_STORED; return; }
    uint32_t left = len;
    while (left && bc >= 8) {  // whole bytes still in the bit buffer
      literal(bits(8));
      if (err) return;
      --left;
    }
    if (left > in_len - ip) { err = E_TRUNCATED; return; }
    if (left > out_len - p) { err = E_OVERRUN; return; }
    while (left) {
      if (budget-- == 0) { err = E_BUDGET; return; }
      const uint32_t n = left < 256u ? left : 256u;
      for (uint32_t k = par.lane(); k < n; k += par.nlanes()) m.ring[(p + k) & RING_MASK] = in[ip + k];
      par.sync();
      p += n;
      ip += n;
      left -= n;
      maybe_flush();
    }
  }
  RI_HD bool fixed_tables() {
    for (int s = par.lane(); s < MAX_LIT; s += par.nlanes()) m.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    par.sync();
    if (!build(m.lens, MAX_LIT, m.lcount, m.loffs, m.lsym, m.lfast, false)) return false;
    for (int s = par.lane(); s < MAX_DIST; s += par.nlanes()) m.lens[s] = 5;
    par.sync();
    return build(m.lens, MAX_DIST, m.dcount, m.doffs, m.dsym, m.dfast, false);
  }
  RI_HD bool dynamic_tables() {
    const int hlit = (int)bits(5) + 257, hdist = (int)bits(5) + 1, hclen = (int)bits(4) + 4;
    if (err) return false;
    if (hlit > 286 || hdist > 30) { err = E_CODES; return false; }
    const char* order = "\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f";
    par.sync();
    for (int i = par.lane(); i < 19; i += par.nlanes()) m.lens[i] = 0;
    par.sync();
    for (int i = 0; i < hclen; ++i) {
      const uint32_t v = bits(3);
      if (par.lane() == 0) m.lens[(int)order[i]] = (uint8_t)v;
    }
    if (err) return false;
    // the code-length code goes in the literal/length tables until the lengths are read
    if (!build(m.lens, 19, m.lcount, m.loffs, m.lsym, m.lfast, true)) return false;
    const int total = hlit + hdist;
    int idx = 0;
    uint8_t prev = 0;
    while (idx < total) {  // every pass stores >= 1 length: at most `total` passes
      const int s = decode(m.lcount, m.lsym, m.lfast);
      if (err) return false;
      int rep = 1;
      uint8_t val;
      if (s < 16) {
        val = (uint8_t)s;
      } else if (s == 16) {
        if (idx == 0) { err = E_CODES; return false; }
        val = prev;
        rep = 3 + (int)bits(2);
      } else if (s == 17) {
        val = 0;
        rep = 3 + (int)bits(3);
      } else {
        val = 0;
        rep = 11 + (int)bits(7);
      }
      if (err) return false;
      if (idx + rep > total) { err = E_CODES; return false; }
      if (par.lane() == 0)
        for (int k = 0; k < rep; ++k) m.lens[idx + k] = val;
      idx += rep;
      prev = val;
    }
    par.sync();
    if (m.lens[256] == 0) { err = E_CODES; return false; }  // no end-of-block code
    if (!build(m.lens, hlit, m.lcount, m.loffs, m.lsym, m.lfast, false)) return false;
    return build(m.lens + hlit, hdist, m.dcount, m.doffs, m.dsym, m.dfast, false);
  }
  RI_HD void codes(size_t& budget) {
    for (;;) {
      if (budget-- == 0) { err = E_BUDGET; return; }
      const int s = decode(m.lcount, m.lsym, m.lfast);
      if (err) return;
      if (s < 256) {
        literal((uint32_t)s);
        if (err) return;
        continue;
      }
      if (s == 256) return;
      const int ls = s - 257;
      if (ls >= 29) { err = E_SYMBOL; return; }
      uint32_t len;
      if (ls < 8) len = 3 + ls;
      else if (ls == 28) len = 258;
      else { const int i = ls - 4, e = i >> 2; len = ((uint32_t)(4 + (i & 3)) << e) + 3 + bits(e); }
      const int ds = decode(m.dcount, m.dsym, m.dfast);
      if (err) return;
      if (ds >= 30) { err = E_SYMBOL; return; }
      uint32_t dist;
      if (ds < 4) dist = 1 + ds;
      else { const int e = (ds - 2) >> 1; dist = ((uint32_t)(2 + (ds & 1)) << e) + 1 + bits(e); }
      if (err) return;
      match(len, dist);
      if (err) return;
    }
  }

  // The whole zlib stream: header, blocks, Adler-32 trailer.  Returns OK only if exactly out_len bytes came out and
  // their Adler-32 matches.
  RI_HD int run() {
    const uint32_t cmf = bits(8), flg = bits(8);
    if (err) return err;
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0) return err = E_HEADER;
    if (flg & 0x20) return err = E_FDICT;
    // every block pass consumes >= 3 input bits, every symbol pass produces >= 1 output byte or ends a block
    size_t budget = out_len + 8 * in_len + 64;
    for (;;) {
      if (budget-- == 0) return err = E_BUDGET;
      const uint32_t final_ = bits(1), type = bits(2);
      if (err) return err;
      if (type == 0) stored(budget);
      else if (type == 3) err = E_BTYPE;
      else if (type == 1 ? fixed_tables() : dynamic_tables()) codes(budget);
      if (err) return err;
      if (final_) break;
    }
    bits(bc & 7);
    uint32_t want = 0;
    for (int k = 0; k < 4; ++k) want = (want << 8) | bits(8);
    if (err) return err;
    if (p != out_len) return err = E_UNDERRUN;
    flush(p - flushed);
    if (want != ((ad_b << 16) | ad_a)) return err = E_ADLER;
    return OK;
  }
};

}  // namespace rinf

#endif  // REVO_INFLATE_H
