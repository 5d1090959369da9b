// The altitude mirror's handle (aog_altmirror), shared by conjugate.hip (its own entry points) and layers.hip
// (aog_install_layer_sum_conjugate reads its surface and origins as one more source).
#pragma once
#include "standalone_handle.h"
#include "../../include/aogym_conjugate.h"

struct aog_altmirror : aog_host::StandaloneHandle<aog_altmirror_config> {   // state: command [B][K] float64
  double* basis = nullptr;     // [K][M M]
  double* fit = nullptr;       // [K][M M]; read only while has_fit
  double* surface = nullptr;   // [B][M M]
  int32_t* origin = nullptr;   // [B][2] zeros
  bool has_fit = false;
};
