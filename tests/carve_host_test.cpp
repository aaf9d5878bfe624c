// Stand-alone host test of Carve (csrc/spg_part.h, the part that needs no HIP): a sizing Carve and a real one agree, the size
// it reports is exactly sufficient, and what it hands out is 256-byte aligned and disjoint.  Built and run by
// tests/test_carve_host.py with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <sys/mman.h>

#include "../superpoint_graph_amd/csrc/spg_part.h"

#define REQUIRE(cond)                                                       \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

namespace {

struct Piece { char* p; size_t bytes; };

// a layout in the shape the units use: a constructor that takes from the Carve; `cells` is the two-variant switch of knn's SegWs
struct Layout {
  std::vector<Piece> pieces;
  Layout(Carve& w, const std::vector<size_t>& sizes, bool cells) {
    for (size_t i = 0; i < sizes.size(); ++i) {
      if (i % 3 == 2 && !cells) continue;      // every third buffer exists only in the `cells` variant
      pieces.push_back({(char*)w.take(sizes[i]), sizes[i]});
    }
  }
};

// the buffer is never touched: it is reserved address space without memory behind it, so it may be larger than the machine's RAM
void check(const std::vector<size_t>& sizes, bool cells) {
  Carve sizing;
  Layout ls(sizing, sizes, cells);
  REQUIRE(sizing.ok);
  for (const Piece& p : ls.pieces) REQUIRE(p.p == nullptr);
  const size_t need = sizing.used();
  REQUIRE(need % 256 == 0);

  const size_t mapped = need + 256;
  char* base = (char*)mmap(nullptr, mapped, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);      // address space only
  REQUIRE(base != (char*)MAP_FAILED && (uintptr_t)base % 256 == 0);
  Carve real(base, need);
  Layout lr(real, sizes, cells);
  REQUIRE(real.ok && real.used() == need && real.left() == 0);
  size_t expect = 0;
  for (size_t i = 0; i < lr.pieces.size(); ++i) {
    const Piece& p = lr.pieces[i];
    REQUIRE(p.p != nullptr && (size_t)(p.p - base) % 256 == 0);
    REQUIRE((size_t)(p.p - base) == expect);                                   // in order, nothing in between but padding
    REQUIRE((size_t)(p.p - base) + p.bytes <= need);
    for (size_t j = 0; j < i; ++j)                                            // disjoint from every earlier one
      REQUIRE(lr.pieces[j].p + lr.pieces[j].bytes <= p.p || p.p + p.bytes <= lr.pieces[j].p);
    expect += align256(p.bytes);
  }
  REQUIRE(expect == need);

  if (need > 0) {
    Carve shy(base, need - 1);
    Layout l1(shy, sizes, cells);
    REQUIRE(!shy.ok && shy.used() < need);
  }
  munmap(base, mapped);
}

}  // namespace

int main() {
  const std::vector<size_t> mixed = {0, 1, 255, 256, 257, (size_t)5 << 30, 3, 1000, 0, 4097};
  check(mixed, true);
  check(mixed, false);
  check({}, true);
  check({1}, true);

  // the variant with more buffers is never the smaller one; a real Carve over a null base is not a sizing one
  Carve a, b;
  Layout la(a, mixed, true), lb(b, mixed, false);
  REQUIRE(a.used() > b.used());
  Carve null_ws(nullptr, 1 << 20);
  REQUIRE(!null_ws.ok && null_ws.take(1) == nullptr && !null_ws.ok);

  REQUIRE(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);
  REQUIRE(bits_of(0) == 1 && bits_of(1) == 1 && bits_of(2) == 2 && bits_of(255) == 8 && bits_of(256) == 9 && bits_of(~0ul) == 64);
  std::puts("carve_host_test: ok");
  return 0;
}
