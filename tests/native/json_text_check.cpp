// Stand-alone check driver of das_amd/csrc/json_text.h (tests/test_atom_docs.py
// compiles it with g++, once plain and once with the address and undefined-
// behaviour sanitizers).  Input (argv[1]): records of a little-endian u32
// length and that many bytes.  Output: per record one line
//   <malformed bytes> <escaped length> <escaped text>
// (the text is ASCII without line breaks by construction).  Exits 1 where the
// measured length and the written bytes disagree.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../das_amd/csrc/json_text.h"

namespace {

struct Get {
  const uint8_t* p;
  uint32_t operator()(uint64_t i) const { return p[i]; }
};

struct Put {
  std::vector<uint8_t>* out;
  uint64_t* next;       // positions must ascend one by one
  bool* ok;
  void operator()(uint64_t at, uint8_t b) const {
    if (at != *next || at >= out->size()) {
      *ok = false;
      return;
    }
    (*out)[at] = b;
    ++*next;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int rc = 0;
  for (;;) {
    uint8_t lb[4];
    if (std::fread(lb, 1, 4, f) != 4) break;
    const uint32_t len = lb[0] | (lb[1] << 8) | (lb[2] << 16) | ((uint32_t)lb[3] << 24);
    // exactly `len` bytes on the heap: a read past the name is the sanitizer's to catch
    std::vector<uint8_t> name(len);
    if (len && std::fread(name.data(), 1, len, f) != len) return 2;
    uint32_t bad = 0;
    const uint64_t n = das::jt_escaped_len(Get{name.data()}, len, &bad);
    uint64_t next = 7;                                  // the text starts where the caller says
    bool ok = true;
    std::vector<uint8_t> shifted(n + 7);
    const uint64_t end = das::jt_escape(Get{name.data()}, len, Put{&shifted, &next, &ok}, 7);
    if (!ok || end != n + 7 || next != end) rc = 1;
    std::printf("%u %llu ", bad, (unsigned long long)n);
    std::fwrite(shifted.data() + 7, 1, (size_t)n, stdout);
    std::fputc('\n', stdout);
  }
  std::fclose(f);
  return rc;
}
