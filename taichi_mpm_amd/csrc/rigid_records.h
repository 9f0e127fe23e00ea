// taichi_mpm_amd/csrc/rigid_records.h — the records of the CPIC rigid coupling that the host fills and the kernels read: plain
// structs, no HIP header.  Included by the device side (k_rigid.h, k_rigid2d.h) and by the host-only set-up (rigid_setup.h).
#pragma once
#include <cstdint>

namespace mpm {
constexpr int MAX_RIGID = 12;                    // GridState::max_num_rigid_bodies (body 0 = background, no surface)
struct RigidBodyDev {
  float pos[3], vel[3], omega[3];
  float R[9];      // body -> world, row-major
  float q[4];      // the same rotation as a quaternion (w, x, y, z)
  float mass, inv_mass;
  float inv_I[9];  // body frame, row-major
  float fric[2];
  float lin_damp, ang_damp;
  float axis[3];   // rotation_axis (all zero: unrestricted)
  int scripted;    // bit 0: position follows a script, bit 1: rotation follows a script
  float tmp_imp[3], tmp_trq[3];  // impulse / torque (about the centre of mass) collected by a transfer (apply_tmp_impulse)
};
struct RigidSample { float off[3]; int body; int elem; };  // boundary particle: offset from the centre of mass, body frame
struct RigidStep {  // what the host knows about a scripted body for one substep: poses at t and t + dt
  int has_pos, has_rot;
  float p0[3], p1[3], q0[4], q1[4];
};
struct RigidSteps { RigidStep s[MAX_RIGID]; };
}  // namespace mpm

namespace mpm2d {
constexpr int MAX_RIGID2 = 12;
struct Rigid2 {
  float pos[2], vel[2], omega, angle;
  float mass, inv_mass, inv_I;
  float fric[2];
  float lin_damp, ang_damp;
  int scripted;
  float tmp_imp[2], tmp_trq;
};
struct Sample2 { float off[2]; int body; int elem; };
struct Step2 { int has_pos, has_rot; float p0[2], p1[2], a0, a1; };  // a0 / a1: radians
struct Steps2 { Step2 s[MAX_RIGID2]; };
}  // namespace mpm2d
