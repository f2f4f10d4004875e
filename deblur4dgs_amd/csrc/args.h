// args.h -- the pointer check of the entry points that name their arguments (observations.hip, feed.hip): host code only.
#pragma once
#include <stdint.h>

#include "host.h"

struct Ptr {
  const void *p;
  const char *name;
  unsigned align;
  bool required;
};

template <int N>
bool pointers_ok(const char *who, const Ptr (&ptrs)[N]) {
  for (const auto &q : ptrs) {
    if (!q.p && q.required) {
      d4gs_set_error("%s: %s is NULL", who, q.name);
      return false;
    }
    if ((uintptr_t)q.p % q.align) {
      d4gs_set_error("%s: %s = %p is misaligned (%u-byte alignment needed)", who, q.name, q.p, q.align);
      return false;
    }
  }
  return true;
}
