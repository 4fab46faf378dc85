// kubebrain_amd/csrc/kdigest.h — the record hash of the batched range digest
// (kb_digest_batch; slab.hip k_digest_tiles). Host and device
// share these functions, so kdigest_hostcheck.cc proves the 16-byte-vector
// formulation the kernel uses against a byte-at-a-time construction of the
// spec on the CPU, and kb_test_digest_record is the host build of it.
//
// All arithmetic is mod 2^64.
//   fmix(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33;
//            x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33
//   word j of a byte string b of length L (0 <= j < ceil(L / 8)): bytes
//   [8j, 8j + 8) as a little-endian u64, bytes at or past L are zero
//   piece(b, S) = sum_j fmix(word_j ^ (S + (j + 1) * G)); empty string: 0
//   record = fmix(fmix(rev ^ S1) + fmix(((klen << 32) | vlen') ^ S2)
//                 + piece(key, SK) + piece(val', SV))
//   vlen' = vlen, val' = val, or 0 and empty under keys_only.
// Every term is independent of every other: lanes hash different words and
// tiles hash different records in any order. A multiset hash for detecting
// divergence and corruption, not an adversarial one.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define KBD_HD __host__ __device__
#else
#define KBD_HD
#endif

namespace kbdigest {

constexpr uint64_t G = 0x9E3779B97F4A7C15ull;
constexpr uint64_t SK = 0x243F6A8885A308D3ull;
constexpr uint64_t SV = 0x13198A2E03707344ull;
constexpr uint64_t S1 = 0xA4093822299F31D0ull;
constexpr uint64_t S2 = 0x082EFA98EC4E6C89ull;

// KB_DIGEST_TILE: rows per tile, clamped like KB_COUNT_TILE (cplan.h)
constexpr int64_t kDefaultTile = 1024;

KBD_HD inline uint64_t fmix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// the salt of word j of a piece salted S
KBD_HD inline uint64_t WordSalt(uint64_t S, uint64_t j) { return S + (j + 1) * G; }

// which bytes of word j belong to a string of len bytes: all of them, the low
// len - 8j of the last partial word, none at or past the end
KBD_HD inline uint64_t TailMask(uint64_t len, uint64_t j) {
  const uint64_t off = j * 8;
  if (off >= len) return 0;
  const uint64_t left = len - off;
  return left >= 8 ? ~0ull : (1ull << (8 * left)) - 1;
}

// the term of word j as memory holds it (whatever lies past len is masked
// off); a word at or past the end has no term, a zero word inside has one
KBD_HD inline uint64_t WordTerm(uint64_t w, uint64_t len, uint64_t j, uint64_t S) {
  if (j * 8 >= len) return 0;
  return fmix((w & TailMask(len, j)) ^ WordSalt(S, j));
}

// one 16-byte vector = words j0 and j0 + 1 of the string; j0 = 2 * (vector
// index), plus 12 for the vectors of a key's spill tail (bytes 96..)
KBD_HD inline uint64_t VecTerms(uint64_t lo, uint64_t hi, uint64_t j0,
                                uint64_t len, uint64_t S) {
  return WordTerm(lo, len, j0, S) + WordTerm(hi, len, j0 + 1, S);
}

// the record finaliser: ksum / vsum are the pieces of key and val'
KBD_HD inline uint64_t Finish(uint64_t rev, uint32_t klen, uint32_t vlenp,
                              uint64_t ksum, uint64_t vsum) {
  return fmix(fmix(rev ^ S1) + fmix((((uint64_t)klen << 32) | vlenp) ^ S2) +
              ksum + vsum);
}

// host form of a piece, vector by vector as the kernel walks it. The staging
// vector is filled with 0xff first, as unfriendly as heap padding can be.
inline uint64_t Piece(const uint8_t* b, size_t len, uint64_t S) {
  uint64_t sum = 0;
  for (size_t v = 0; v * 16 < len; ++v) {
    uint64_t w[2] = {~0ull, ~0ull};
    const size_t left = len - v * 16;
    memcpy(w, b + v * 16, left < 16 ? left : 16);  // little-endian hosts
    sum += VecTerms(w[0], w[1], 2 * v, len, S);
  }
  return sum;
}

inline uint64_t Record(uint64_t rev, const uint8_t* key, size_t klen,
                       const uint8_t* val, size_t vlen, bool keys_only) {
  const size_t vl = keys_only ? 0 : vlen;
  return Finish(rev, (uint32_t)klen, (uint32_t)vl, Piece(key, klen, SK),
                Piece(val, vl, SV));
}

}  // namespace kbdigest
