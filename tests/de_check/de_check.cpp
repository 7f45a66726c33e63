// Reader safety of the oracle's bincode reader De (oracle/nizk.hpp), stand-alone: built with ASan + UBSan by
// tests/test_de_check.py and run as its own process. Test infrastructure only.
//
//   de_check <proof file> <offsets file>
//
// The offsets file holds one line per field of the typed map (tests/proof_layout.py): "b <offset>" for a field
// boundary, "l <offset>" for the start of a Vec length. The honest proof must parse and re-serialise to itself; every
// truncation at a field boundary must be Malformed; the proof with each length set to 0, length + 1 and 2^63 must be
// Malformed, or parse cleanly only as a shorter proof followed by trailing bytes (which SNARKProof::de reports as
// Malformed as well). Anything else, and any sanitizer report, is a failure. Exit 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "snark.hpp"

using namespace orc;

// 0 = parsed, 1 = Malformed
static int parse(const std::vector<uint8_t>& b, std::vector<uint8_t>* out = nullptr) {
  try {
    // an exact-size heap copy: a read past the end is a heap-buffer-overflow under ASan
    std::vector<uint8_t> copy(b);
    copy.shrink_to_fit();
    De d(copy.data(), copy.size());
    SNARKProof pf = SNARKProof::de(d);
    if (out) {
      Ser s;
      pf.ser(s);
      *out = s.b;
    }
    return 0;
  } catch (const Malformed&) {
    return 1;
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: de_check <proof file> <offsets file>\n");
    return 2;
  }
  std::ifstream pfile(argv[1], std::ios::binary);
  std::vector<uint8_t> proof((std::istreambuf_iterator<char>(pfile)), std::istreambuf_iterator<char>());
  std::ifstream ofile(argv[2]);
  std::vector<size_t> bounds, lens;
  std::string kind;
  size_t off;
  while (ofile >> kind >> off) (kind == "l" ? lens : bounds).push_back(off);
  if (proof.empty() || bounds.empty() || lens.empty()) {
    fprintf(stderr, "de_check: empty input\n");
    return 2;
  }
  int bad = 0;
  std::vector<uint8_t> again;
  if (parse(proof, &again) != 0 || again != proof) {
    fprintf(stderr, "de_check: the honest proof does not round-trip\n");
    bad++;
  }
  for (size_t b : bounds) {
    if (b >= proof.size()) continue;  // the end of the last field is the whole proof
    std::vector<uint8_t> cut(proof.begin(), proof.begin() + b);
    if (parse(cut) != 1) {
      fprintf(stderr, "de_check: truncation at %zu parsed\n", b);
      bad++;
    }
  }
  for (size_t l : lens) {
    if (l + 8 > proof.size()) {
      fprintf(stderr, "de_check: length offset %zu outside the proof\n", l);
      return 2;
    }
    uint64_t n = 0;
    for (int i = 0; i < 8; i++) n |= (uint64_t)proof[l + i] << (8 * i);
    const uint64_t vals[3] = {0, n + 1, (uint64_t)1 << 63};
    for (uint64_t v : vals) {
      if (v == n) continue;
      std::vector<uint8_t> m(proof);
      for (int i = 0; i < 8; i++) m[l + i] = (uint8_t)(v >> (8 * i));
      if (parse(m) != 1) {  // a changed length moves every later field: the bytes cannot add up again
        fprintf(stderr, "de_check: length at %zu set to %llu parsed\n", l, (unsigned long long)v);
        bad++;
      }
    }
  }
  printf("de_check: %zu truncations, %zu lengths x 3, %d failures\n", bounds.size(), lens.size(), bad);
  return bad ? 1 : 0;
}
