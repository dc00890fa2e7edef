// kfn_ckpt.hip -- host side of reading TensorFlow checkpoints: CRC32C of the table blocks and tensor bytes.
//
// A tf.train.Saver V2 checkpoint (`model.ckpt-<step>.index` + `.data-*-of-*`) checksums every table block and every tensor
// with CRC32C (Castagnoli, reflected polynomial 0x82F63B78).  kfnet_amd/checkpoint.py parses the files and calls this for
// the bytes it reads: about 100 MB for a full KFNet checkpoint, which a pure-Python CRC would take tens of seconds over.
// Two implementations that give the same bits: the SSE4.2 `crc32` instruction when cpuid reports it (chosen once, at run
// time), else a slicing-by-8 table.  Host code only: no kernel, no device access.
//
// Self-contained on purpose (the library header and the C++ standard library only), so a host compiler can build this file
// on its own: tests/test_checkpoint_host.py compares the two implementations bit for bit that way.
#include "../../include/kfnet_hip.h"

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace kfn {
int fail(int code, const char* fmt, ...);   // kfn_runtime.hip: thread-local text of kfn_last_error()
}

namespace {

constexpr uint32_t kPoly = 0x82F63B78u;   // CRC-32C, bit-reflected

struct Crc32cTables {
  uint32_t t[8][256];
  Crc32cTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kPoly & (0u - (c & 1u)));
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFFu];
  }
};

const Crc32cTables& tables() {
  static const Crc32cTables tab;   // thread-safe one-time initialisation
  return tab;
}

// Both take and return the raw register (pre-/post-inversion is the caller's).
uint32_t crc32c_table(uint32_t c, const unsigned char* p, size_t n) {
  const Crc32cTables& T = tables();
  while (n && (reinterpret_cast<uintptr_t>(p) & 7u)) {
    c = (c >> 8) ^ T.t[0][(c ^ *p++) & 0xFFu];
    --n;
  }
  while (n >= 8) {
    uint64_t w;
    std::memcpy(&w, p, 8);   // little-endian host (x86-64; the checkpoint format is little-endian too)
    w ^= c;
    c = T.t[7][w & 0xFFu] ^ T.t[6][(w >> 8) & 0xFFu] ^ T.t[5][(w >> 16) & 0xFFu] ^ T.t[4][(w >> 24) & 0xFFu] ^
        T.t[3][(w >> 32) & 0xFFu] ^ T.t[2][(w >> 40) & 0xFFu] ^ T.t[1][(w >> 48) & 0xFFu] ^ T.t[0][w >> 56];
    p += 8;
    n -= 8;
  }
  while (n--) c = (c >> 8) ^ T.t[0][(c ^ *p++) & 0xFFu];
  return c;
}

#if defined(__x86_64__)
__attribute__((target("sse4.2"))) uint32_t crc32c_sse42(uint32_t c, const unsigned char* p, size_t n) {
  while (n && (reinterpret_cast<uintptr_t>(p) & 7u)) {
    c = __builtin_ia32_crc32qi(c, *p++);
    --n;
  }
  uint64_t c64 = c;
  while (n >= 8) {
    uint64_t w;
    std::memcpy(&w, p, 8);
    c64 = __builtin_ia32_crc32di(c64, w);
    p += 8;
    n -= 8;
  }
  c = (uint32_t)c64;
  while (n--) c = __builtin_ia32_crc32qi(c, *p++);
  return c;
}

bool have_sse42() {
  static const bool yes = __builtin_cpu_supports("sse4.2");
  return yes;
}
#else
uint32_t crc32c_sse42(uint32_t c, const unsigned char* p, size_t n) { return crc32c_table(c, p, n); }
bool have_sse42() { return false; }
#endif

}  // namespace

// Extends *crc over n bytes (CRC-32C with the usual ~0 pre- and post-inversion): *crc == 0 starts a checksum, and
// feeding a buffer in pieces gives the same value as one call over all of it.
extern "C" int kfn_crc32c(const void* data, size_t n, uint32_t* crc) {
  if (!crc || (n && !data)) return kfn::fail(KFN_ERR_ARG, "kfn_crc32c: null %s", crc ? "data" : "crc");
  const unsigned char* p = static_cast<const unsigned char*>(data);
  const uint32_t c = ~*crc;
  *crc = ~(have_sse42() ? crc32c_sse42(c, p, n) : crc32c_table(c, p, n));
  return KFN_OK;
}
