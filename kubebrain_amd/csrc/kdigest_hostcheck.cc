// kubebrain_amd/csrc/kdigest_hostcheck.cc — stand-alone CPU check of the
// record hash of kb_digest_batch (kdigest.h): the 16-byte-vector formulation
// k_digest_tiles uses (two words per vector, a word index derived from the
// vector index, a masked tail, the key split into its 96-byte column row and
// a spill tail whose word index continues at 12, 16 lanes taking the vectors
// round-robin) against a naive byte-at-a-time construction of the spec, for
// every key length in {0,1,7,8,9,95,96,97,104,300,4096} and every value
// length in {0,1,15,16,17,255,256,257,4095,4097}, with and without
// keys_only. The sources are laid out as the slab holds them (column row,
// spill tail and value each padded to 16) with 0xa5 in every padding byte,
// in buffers of exactly the padded size, so a read past an extent is a
// sanitizer report and a padding byte that reaches the hash is a mismatch.
// No HIP, no store; meant to be built with sanitizers:
//   make -C kubebrain_amd/csrc digest-hostcheck        (plain)
//   make -C kubebrain_amd/csrc digest-hostcheck-asan   (-fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kdigest.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

using namespace kbdigest;

constexpr size_t KEYW = 96;

// the spec, byte at a time: word j gathers bytes [8j, 8j + 8) below L
static uint64_t naive_piece(const std::vector<uint8_t>& b, uint64_t S) {
  uint64_t sum = 0;
  for (size_t j = 0; j * 8 < b.size(); ++j) {
    uint64_t w = 0;
    for (size_t k = 0; k < 8; ++k)
      if (j * 8 + k < b.size()) w |= (uint64_t)b[j * 8 + k] << (8 * k);
    uint64_t x = w ^ (S + (j + 1) * G);
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    sum += x;
  }
  return sum;
}

static uint64_t naive_record(uint64_t rev, const std::vector<uint8_t>& key,
                             const std::vector<uint8_t>& val, bool konly) {
  const std::vector<uint8_t> none;
  const std::vector<uint8_t>& v = konly ? none : val;
  return fmix(fmix(rev ^ S1) +
              fmix((((uint64_t)key.size() << 32) | (uint64_t)v.size()) ^ S2) +
              naive_piece(key, SK) + naive_piece(v, SV));
}

static std::vector<uint8_t> padded(const uint8_t* b, size_t len, size_t extent) {
  std::vector<uint8_t> o(extent, 0xa5);
  for (size_t i = 0; i < len; ++i) o[i] = b[i];
  return o;
}

static void load16(const std::vector<uint8_t>& src, size_t v, uint64_t w[2]) {
  if (v * 16 + 16 > src.size()) abort();  // the kernel's extent checks forbid it
  memcpy(w, src.data() + v * 16, 16);
}

// the walk of one 16-lane group of k_digest_tiles over one record
static uint64_t vector_record(uint64_t rev, const std::vector<uint8_t>& key,
                              const std::vector<uint8_t>& val, bool konly) {
  const size_t klen = key.size(), vlen = konly ? 0 : val.size();
  const size_t kin = klen < KEYW ? klen : KEYW;
  const std::vector<uint8_t> col = padded(key.data(), kin, KEYW);
  const std::vector<uint8_t> tail =
      padded(key.data() + kin, klen - kin, (klen - kin + 15) & ~(size_t)15);
  const std::vector<uint8_t> heap =
      padded(val.data(), vlen, (vlen + 15) & ~(size_t)15);
  uint64_t lane_sum[16] = {0};
  uint64_t w[2];
  for (size_t gl = 0; gl < 16; ++gl) {
    uint64_t ks = 0, vs = 0;
    if (gl < 6 && gl * 16 < kin) {  // cut at ceil(klen / 8) words, not at zeros
      load16(col, gl, w);
      ks += VecTerms(w[0], w[1], 2 * gl, klen, SK);
    }
    for (size_t t = gl; t * 16 < klen - kin; t += 16) {
      load16(tail, t, w);
      ks += VecTerms(w[0], w[1], 12 + 2 * t, klen, SK);
    }
    for (size_t v = gl; v * 16 < vlen; v += 16) {
      load16(heap, v, w);
      vs += VecTerms(w[0], w[1], 2 * v, vlen, SV);
    }
    lane_sum[gl] = ks + vs;
  }
  for (int d = 8; d >= 1; d >>= 1)  // the 16-lane xor-shuffle sum
    for (int l = 0; l < 16; ++l)
      if (!(l & d)) {
        const uint64_t s = lane_sum[l] + lane_sum[l ^ d];
        lane_sum[l] = lane_sum[l ^ d] = s;
      }
  return Finish(rev, (uint32_t)klen, (uint32_t)vlen, lane_sum[0], 0);
}

int main() {
  const size_t klens[] = {0, 1, 7, 8, 9, 95, 96, 97, 104, 300, 4096};
  const size_t vlens[] = {0, 1, 15, 16, 17, 255, 256, 257, 4095, 4097};
  uint64_t seed = 0x1234567;
  auto next = [&]() {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint8_t)(seed >> 56);
  };
  int64_t cases = 0;
  // mask and salt edges
  CHECK(TailMask(0, 0) == 0 && TailMask(8, 0) == ~0ull && TailMask(8, 1) == 0);
  CHECK(TailMask(9, 1) == 0xff && TailMask(15, 1) == 0x00ffffffffffffffull);
  CHECK(WordSalt(SK, 0) == SK + G && WordTerm(~0ull, 8, 1, SK) == 0);
  CHECK(fmix(0) == 0 && fmix(1) == 0xb456bcfc34c2cb2cull);
  for (size_t kl : klens)
    for (size_t vl : vlens)
      for (int fill = 0; fill < 3; ++fill) {
        // random bytes, all zero (a zero word still has a term), all 0xff
        std::vector<uint8_t> key(kl), val(vl);
        for (auto& b : key) b = fill == 0 ? next() : fill == 1 ? 0 : 0xff;
        for (auto& b : val) b = fill == 0 ? next() : fill == 1 ? 0 : 0xff;
        const uint64_t rev = fill == 0 ? seed : (uint64_t)fill;
        for (int konly = 0; konly < 2; ++konly) {
          const uint64_t want = naive_record(rev, key, val, konly != 0);
          CHECK(vector_record(rev, key, val, konly != 0) == want);
          CHECK(Record(rev, key.data(), kl, val.data(), vl, konly != 0) == want);
          ++cases;
        }
        // keys_only ignores the value bytes, not the key or the revision
        CHECK(naive_record(rev, key, val, true) ==
              naive_record(rev, key, std::vector<uint8_t>(), false));
        if (vl) CHECK(naive_record(rev, key, val, true) !=
                      naive_record(rev, key, val, false));
        CHECK(Record(rev + 1, key.data(), kl, val.data(), vl, false) !=
              Record(rev, key.data(), kl, val.data(), vl, false));
      }
  // a trailing zero byte changes the hash (the lengths and word count differ)
  {
    const uint8_t a[9] = {'k', 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(Record(5, a, 1, a, 0, false) != Record(5, a, 2, a, 0, false));
    CHECK(Record(5, a, 8, a, 0, false) != Record(5, a, 9, a, 0, false));
    CHECK(Record(5, a, 1, a, 8, false) != Record(5, a, 1, a, 9, false));
  }
  printf("kdigest hostcheck OK: %lld cases\n", (long long)cases);
  return 0;
}
