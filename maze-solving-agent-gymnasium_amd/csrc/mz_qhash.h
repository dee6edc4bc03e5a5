// mz_qhash.h — the probe and the claim of the hashed Q-tables (mz_qtab.h's Hashed<W>: one 4-wide
// row per slot for Q, an A row and a B row per slot for double Q). Only the keys are touched here:
// int32 [C] per table, -1 = empty, slot0 = (uint32(key) * 0x9E3779B1u) >> shift, then +1 mod C.
// Every loop runs at most C iterations, so a full table terminates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int QH_FOUND = 1, QH_EMPTY = 0, QH_FULL = -1;
constexpr int QH_MAX_BLOCKS = 1 << 20;  // rehash: a grid-stride loop beyond this many workgroups

__device__ inline uint32_t qhash_slot0(int32_t key, int shift) {
  return ((uint32_t)key * 0x9E3779B1u) >> shift;
}

// Read-only probe of one table's keys: QH_FOUND (slot holds key), QH_EMPTY (slot is the empty slot
// that ends the chain) or QH_FULL (C slots seen, none empty, none the key).
__device__ inline int qhash_probe(const int32_t* keys, uint32_t C, int shift, int32_t key,
                                  uint32_t& slot) {
  uint32_t p = qhash_slot0(key, shift);
  for (uint32_t it = 0; it < C; ++it) {
    const int32_t k = keys[p];
    if (k == key || k == -1) {
      slot = p;
      return k == key ? QH_FOUND : QH_EMPTY;
    }
    p = (p + 1) & (C - 1);
  }
  return QH_FULL;
}

// Find or insert under concurrent inserts: true with the key's slot, false if the table is full.
// fresh: this lane claimed the slot.
__device__ inline bool qhash_claim(int32_t* keys, uint32_t C, int shift, int32_t key,
                                   uint32_t& slot, bool& fresh) {
  uint32_t p = qhash_slot0(key, shift);
  fresh = false;
  for (uint32_t it = 0; it < C; ++it) {
    int32_t k = keys[p];
    if (k == -1) {
      k = atomicCAS(keys + p, -1, key);  // the slot's key as it stood
      if (k == -1) {
        fresh = true;
        k = key;
      }
    }
    if (k == key) {
      slot = p;
      return true;
    }
    p = (p + 1) & (C - 1);
  }
  return false;
}

}  // namespace
