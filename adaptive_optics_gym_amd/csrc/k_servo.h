// K22: the mirror servo (aog_servo_*): per (env, actuator) a delay line of the commanded actions, a drive clip, a first-order response
// and a stuck-actuator override between the action a policy commands and the action the mirror receives.
#pragma once
#include "k_common.h"

namespace aog {

// State: y [B][A] float64, the handle's call counter n (uint64), ring [B][R][A] float32, R = max_latency + 2 — the checkpoint blob as it
// stands.  One thread per (env, actuator).  The call that finds the counter at n writes slot n mod R; a_{n-k} is slot (n - k) mod R.
//   c = a_{n-d}  (f == 0)   or   ((1 - f) a_{n-d}) + (f a_{n-d-1});   clip to [-stroke, stroke] unless stroke is +inf;
//   y = c  (response == 1)   or   y + (response (c - y));   out = stuck ? stuck_value : (float)y
// Every product, difference and sum is one rounded float64 operation (mul_rn / add_rn of k_common.h: never one fma; a difference is the
// sum with the negated operand, which rounds alike): a host replay is bit-exact.  No thread reads the counter: the host keeps it and
// passes slot = n mod R and next = n + 1; thread 0 stores `next` for aog_servo_get_state (a word no thread of this launch reads).
struct ServoArgs {
  double* y;                          // [B][A]
  unsigned long long* counter;
  float* ring;                        // [B][R][A]
  const int* delay;                   // [B] d = floor(latency)
  const double* frac;                 // [B] f = latency - d
  const double* response;             // [B]
  const double* stroke;               // [B] (+inf: none)
  const uint8_t* stuck;               // [B][A]
  const float* stuck_value;           // [B][A]
  const float* in;                    // [B][A]
  const uint8_t* mask;                // nullable [B]
  float* out;                         // [B][A]
  int B, A, R, slot;
  unsigned long long next;
};

__global__ __launch_bounds__(256) void k_servo_apply(ServoArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *a.counter = a.next;
  if (i >= a.B * a.A) return;
  const int env = i / a.A, j = i - env * a.A;
  if (a.mask && !a.mask[env]) return;
  float* ring = a.ring + (size_t)env * a.R * a.A + j;
  const float cmd = a.in[i];
  ring[(size_t)a.slot * a.A] = cmd;
  const int d = a.delay[env];
  const double f = a.frac[env];
  // (d = 0 reads the command just stored: from the register, not through memory)
  int s0 = a.slot - d;
  s0 += s0 < 0 ? a.R : 0;
  double c = d == 0 ? (double)cmd : (double)ring[(size_t)s0 * a.A];
  if (f != 0.0) {
    int s1 = s0 - 1;
    s1 += s1 < 0 ? a.R : 0;
    c = add_rn(mul_rn(add_rn(1.0, -f), c), mul_rn(f, (double)ring[(size_t)s1 * a.A]));
  }
  const double stroke = a.stroke[env];
  if (stroke < __builtin_huge_val()) {
    c = c < -stroke ? -stroke : c;
    c = c > stroke ? stroke : c;
  }
  const double r = a.response[env];
  double y = c;
  if (r != 1.0) {
    const double y0 = a.y[i];
    y = add_rn(y0, mul_rn(r, add_rn(c, -y0)));
  }
  a.y[i] = y;
  a.out[i] = a.stuck[i] ? a.stuck_value[i] : (float)y;
}

// ring and y of the selected envs to the rest command 0
__global__ __launch_bounds__(256) void k_servo_reset(double* y, float* ring, const uint8_t* mask, int B, int A, int R) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * A) return;
  const int env = i / A, j = i - env * A;
  if (mask && !mask[env]) return;
  y[i] = 0.0;
  float* row = ring + (size_t)env * R * A + j;
  for (int s = 0; s < R; ++s) row[(size_t)s * A] = 0.f;
}

}  // namespace aog
