// lf_sensor_event.h -- the sensor as a mirror of the geometric lens (lf_set_sensor_ghosts; DESIGN.md section 4, "sensor
// ghosts"): a ray that travels +z behind the rear element is carried to the plane z = z_sensor and reflected specularly,
// d_z -> -d_z; one that lands outside the sensor's rectangle |X| <= xmax, |Y| <= ymax is lost.  ONE definition for the host
// (lf_sensor_mirror_event) and the kernels (lf_march_sensor.hip): every multiply-add an explicit fmaf, the division the IEEE
// one (-fhip-fp32-correctly-rounded-divide-sqrt, -ffp-contract=off), so that both sides agree bit for bit -- as lf_asphere.h's
// event does.  Nothing here is part of the ABI.
#pragma once

#include <cmath>

#include "lf_internal.h"
#include "lf_march_events.h"

namespace lfm {

// The Ray conventions of surface_event (lf_march_events.h): the position relative to the vertex of the interface the ray
// sits on, dzv = that vertex's z minus the sensor plane's, K = n d.  Leaves the ray ON the plane (hz = 0, as after the stop
// and at a sample's start) with the mirrored direction; returns whether it landed inside the rectangle (false for a NaN).
__host__ __device__ inline bool lf_sensor_mirror(float& px, float& py, float& hz, float& r2, float& dx, float& dy, float& dz,
                                                 float dzv, float xmax, float ymax) {
  const float t = -(hz + dzv) / dz;
  const float x = fmaf(t, dx, px), y = fmaf(t, dy, py);
  px = x; py = y; hz = 0.0f;
  r2 = fmaf(x, x, y * y);
  dz = -dz;
  return fabsf(x) <= xmax && fabsf(y) <= ymax;
}

// The event of a marching wave: the stop event's interface (a flat plane, one liveness mask).  W = true multiplies the
// weight by the sensor's reflectance at the row's wavelength -- one number, whatever the angle.
template <bool W>
__device__ __forceinline__ lanemask sensor_event(Ray& r, float dzv, float xmax, float ymax, float reflectance) {
  const bool in = lf_sensor_mirror(r.px, r.py, r.hz, r.r2, r.dx, r.dy, r.dz, dzv, xmax, ymax);
  if (W) r.wn *= reflectance;
  return __ballot(in);
}

}  // namespace lfm
