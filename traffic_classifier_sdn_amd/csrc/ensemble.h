// Kernel-argument block of ensemble_vote_kernel, shared by the kernel TU and
// the host-only binding TU.  Everything a launch needs about its members is
// in here BY VALUE: there is no device-side pointer array to fill, so the
// launch needs no copy and no allocation and captures into a graph.
#pragma once

#define ENS_MAX_M 8  // members
#define ENS_MAX_C 8  // classes, of a member and of the ensemble

struct EnsembleArgs {
  const float* p[ENS_MAX_M];                    // [n, cm[m]] f32, 16-B aligned
  float w[ENS_MAX_M];                           // normalised weights
  unsigned char cm[ENS_MAX_M];                  // member class counts
  unsigned char map[ENS_MAX_M * ENS_MAX_C];     // member column -> ensemble column
  int M;
};
