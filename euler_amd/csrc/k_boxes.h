// k_boxes.h — a list of at most 64 boxes on the device, the way the force boxes (k_forcing.hip) and the heat boxes (k_heat.hip) keep it: the boxes as the caller
// gave them - any record that begins with x0, y0, x1, y1 - and behind them the TILE TABLE (eu_force_tiles, euler_host.c): one entry per 64 x 64 tile that a box
// touches, with those boxes as a bit set.  One workgroup takes one entry, so the set and every test on it are uniform across the workgroup.
#pragma once
#include "euler_dev.h"

// boxes[0 .. max_boxes) and the tile table behind them into buf (grown on demand; k_observe.hip), the copy waited for; *ntiles: the table's entries
int eu_box_table_upload(euler_sim* S, const char* who, eu_devbuf* buf, const void* boxes, int32_t n, size_t box_bytes, int32_t max_boxes, unsigned int* ntiles);

#ifdef __HIPCC__
// (x, y) lies in some box of the set: only then is the cell inside the interior and may anything of it be read
template <class BOX>
__device__ __forceinline__ bool eu_boxes_hold(const BOX* __restrict__ boxes, unsigned long long set, int x, int y) {
  bool in = false;
  for (unsigned long long m = set; m; m &= m - 1) {
    const BOX b = boxes[__ffsll((long long)m) - 1];
    in |= x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1;
  }
  return in;
}
// (The walk that applies the boxes - every box of the set that holds the cell, bit 0 first: the list order - stays written out in k_force_boxes and k_heat_boxes:
// through a shared "for each" helper k_force_boxes came out 4 % slower with one box over the interior, profiles/transport_refactor.md.)
#endif
