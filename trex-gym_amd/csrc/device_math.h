// The small 3-vector / 3x3 algebra of the device code, written once: the step body, the dynamics queries, the utility kernels
// and the renderer all take it from here. Matrices are row-major float[9]; every output may alias an input.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void cross3(const float *a, const float *b, float *o) {
  const float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}
__device__ __forceinline__ float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void matvec3(const float *m, const float *v, float *o) {
  const float x = m[0] * v[0] + m[1] * v[1] + m[2] * v[2];
  const float y = m[3] * v[0] + m[4] * v[1] + m[5] * v[2];
  const float z = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
  o[0] = x; o[1] = y; o[2] = z;
}
__device__ __forceinline__ void matmul3(const float *a, const float *b, float *o) {
  float t[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) t[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
#pragma unroll
  for (int i = 0; i < 9; i++) o[i] = t[i];
}
// symmetric 3x3 (xx xy xz yy yz zz) times vector
__device__ __forceinline__ void sym3_mul(const float *s, const float *v, float *o) {
  const float x = s[0] * v[0] + s[1] * v[1] + s[2] * v[2];
  const float y = s[1] * v[0] + s[3] * v[1] + s[4] * v[2];
  const float z = s[2] * v[0] + s[4] * v[1] + s[5] * v[2];
  o[0] = x; o[1] = y; o[2] = z;
}
// unit quaternion xyzw -> rotation matrix
__device__ __forceinline__ void quat_to_mat(const float *q, float *m) {
  const float x = q[0], y = q[1], z = q[2], w = q[3];
  m[0] = 1 - 2 * (y * y + z * z); m[1] = 2 * (x * y - z * w); m[2] = 2 * (x * z + y * w);
  m[3] = 2 * (x * y + z * w); m[4] = 1 - 2 * (x * x + z * z); m[5] = 2 * (y * z - x * w);
  m[6] = 2 * (x * z - y * w); m[7] = 2 * (y * z + x * w); m[8] = 1 - 2 * (x * x + y * y);
}
// The rotation of a hinge at angle q about its (unit) axis, Rodrigues' formula, from c = cosf(q) and s = sinf(q):
// out = jrot * Rot(axis, q), the joint's pose in its parent's frame - or Rot(axis, q) alone where jrot is null (a caller that
// composes (R * jrot) * Rot itself). (The caller takes the cosine and sine: with the two calls in here the compiler orders
// their expansions differently after inlining, and every kernel that uses it changes its instruction schedule.)
__device__ __forceinline__ void hinge_rot(const float *jrot, const float *axis, float c, float s, float *out) {
  const float t = 1.f - c;
  float rq[9];
  rq[0] = t * axis[0] * axis[0] + c;           rq[1] = t * axis[0] * axis[1] - s * axis[2]; rq[2] = t * axis[0] * axis[2] + s * axis[1];
  rq[3] = t * axis[0] * axis[1] + s * axis[2]; rq[4] = t * axis[1] * axis[1] + c;           rq[5] = t * axis[1] * axis[2] - s * axis[0];
  rq[6] = t * axis[0] * axis[2] - s * axis[1]; rq[7] = t * axis[1] * axis[2] + s * axis[0]; rq[8] = t * axis[2] * axis[2] + c;
  if (jrot) {
    matmul3(jrot, rq, out);
  } else {
#pragma unroll
    for (int i = 0; i < 9; i++) out[i] = rq[i];
  }
}
