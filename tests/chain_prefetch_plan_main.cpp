// Host check of the weight-prefetch plan of csrc/gemm_chain.hip (built and run by tests/test_chain_prefetch_plan.py with
// -fsanitize=address,undefined).  It includes the header the kernel includes and calls the functions the kernel calls - pf_thread
// and pf_line - for every thread of every block, and checks against buffers of exactly the size chain_pack_weights allocates
// (nk x NW x ntg x 2048 bytes per unit) that
//   * the blocks that share an XCD (block % 8; ranks block / 8) together touch every 128-byte line of every unit exactly once,
//   * every touched 4 bytes lie inside the unit's buffer (the program really reads them: the sanitizer sees an overrun),
//   * the LDS landing area of the requests lies inside what the launch asks for, for 1 - 3 strips per panel.
// An out-of-range request on the device would be a fault; this is where that is excluded.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemm_chain_prefetch.h"

using namespace aimnet;
using namespace aimnet::chain;

static long g_checked = 0;

#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      std::fprintf(stderr, "FAILED: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");          \
      std::exit(1);                        \
    }                                      \
  } while (0)

template <class S>
static void check_shape(int id, int grid) {
  constexpr int NU = n_units<S>(), NTH = 64 * S::NW;
  // one heap buffer per unit, exactly as large as the packed stream
  std::vector<std::vector<unsigned char>> buf(NU);
  int total = 0;
  for (int u = 0; u < NU; ++u) {
    // chain_pack_weights (gemm_chain.hip) allocates nk * nw * nt * 2 planes * 64 lanes * 8 sixteen-bit elements per unit
    const int bytes = unit_nk<S>(u) * S::NW * unit_nt<S>(u) * 2 * 64 * 8 * 2;
    CHECK(bytes == unit_bytes<S>(u) && bytes % CHAIN_PF_LINE == 0, "shape %d unit %d: %d bytes", id, u, bytes);
    CHECK(unit_lines<S>(u) % 64 == 0, "shape %d unit %d: a wave's 64 lines would straddle a unit", id, u);
    buf[u].assign(bytes, 0);
    total += unit_lines<S>(u);
  }
  CHECK(total == stream_lines<S>(), "shape %d: stream_lines", id);
  CHECK(pf_line<S>(-1).unit == NU && pf_line<S>(total).unit == NU, "shape %d: lines outside the stream must map to no unit", id);
  const int n_xcd = grid < CHAIN_PF_XCDS ? grid : CHAIN_PF_XCDS;
  int blocks_seen = 0;
  for (int xcd = 0; xcd < n_xcd; ++xcd) {
    for (auto& b : buf) b.assign(b.size(), 0);
    for (int block = xcd; block < grid; block += CHAIN_PF_XCDS) {
      ++blocks_seen;
      for (int tid = 0; tid < NTH; ++tid) {
        const PfThread t = pf_thread(grid, block, tid, NTH);
        CHECK(t.first >= 0 && t.stride >= NTH, "shape %d grid %d block %d: stride %d", id, grid, block, t.stride);
        for (int g = t.first; g < stream_lines<S>(); g += t.stride) {  // the kernel's loop
          const PfLine pl = pf_line<S>(g);
          CHECK(pl.unit >= 0 && pl.unit < NU, "shape %d grid %d: line %d -> unit %d", id, grid, g, pl.unit);
          CHECK(pl.offset % CHAIN_PF_LINE == 0 && (size_t)pl.offset + 4 <= buf[pl.unit].size(), "shape %d grid %d block %d thread %d: offset %u of unit %d (%zu bytes)",
                id, grid, block, tid, pl.offset, pl.unit, buf[pl.unit].size());
          unsigned char* p = buf[pl.unit].data() + pl.offset;  // the four bytes the request reads
          CHECK(p[0] == 0 && p[1] == 0 && p[2] == 0 && p[3] == 0, "shape %d grid %d xcd %d: line %u of unit %d requested twice", id, grid, xcd,
                pl.offset / CHAIN_PF_LINE, pl.unit);
          p[0] = p[1] = p[2] = p[3] = 1;
          ++g_checked;
        }
      }
    }
    for (int u = 0; u < NU; ++u)
      for (size_t o = 0; o < buf[u].size(); o += CHAIN_PF_LINE)
        CHECK(buf[u][o] == 1, "shape %d grid %d xcd %d: line %zu of unit %d is not requested", id, grid, xcd, o / CHAIN_PF_LINE, u);
  }
  CHECK(blocks_seen == grid, "grid %d: %d blocks visited", grid, blocks_seen);
  // where the launcher issues the requests by default: no thread of any XCD has more than CHAIN_PF_MAX_LINES lines
  int most = 0;
  for (int block = 0; block < grid; ++block) {
    const PfThread t = pf_thread(grid, block, 0, NTH);
    int n = 0;
    for (int g = t.first; g < stream_lines<S>(); g += t.stride) ++n;
    most = n > most ? n : most;
  }
  CHECK(pf_pays<S>(grid) == (grid >= CHAIN_PF_XCDS && most <= CHAIN_PF_MAX_LINES), "shape %d grid %d: pf_pays with %d lines per thread", id, grid, most);
}

int main() {
  const int grids[] = {1, 7, 8, 9, 210, 256, 775};
  // the plan has no strip parameter (a block has 64 NW threads whatever its panel height): grids and shapes are checked once;
  // what depends on the strips per panel (1 - 3) is where the requests land in LDS
  for (int strips = 1; strips <= CH_MAX_SM; ++strips) {
    CHECK(chain_pf_lds_offset(strips) == CHAIN_MAX_KB * strips * 2048, "LDS offset for %d strips", strips);
    CHECK(chain_pf_lds_offset(strips) + 64 * 4 <= chain_lds_bytes(strips) && chain_lds_bytes(strips) <= CHAIN_LDS_LIMIT, "LDS landing area for %d strips", strips);
  }
  for (int grid : grids)
    static_for<0, N_SHAPES>([&](auto s_c) { check_shape<Shape<decltype(s_c)::value>>(decltype(s_c)::value, grid); });
  for (int grid : grids) {
    int n = 0;
    for (int xcd = 0; xcd < CHAIN_PF_XCDS; ++xcd) n += pf_blocks_on_xcd(grid, xcd);
    CHECK(n == grid, "grid %d: blocks per XCD sum to %d", grid, n);
  }
  std::printf("chain prefetch plan ok: %ld requests checked\n", g_checked);
  return 0;
}
