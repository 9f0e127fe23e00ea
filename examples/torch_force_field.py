"""A force field written in torch, applied to the particles on the device: a small sand column is stirred by a swirl around the
vertical axis through the middle of the box.  Before every frame the positions and velocities come out as torch tensors
(Simulation3D.get_particle_tensors), three lines of torch add dt * a(x) to the velocities, and the velocities go back
(set_particle_tensors) — no particle record and no field row passes through host memory, which the counter printed at the end
shows: it holds what add_particles uploaded and nothing more.  Needs an MI355X and torch.

    python examples/torch_force_field.py [frames] [res]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taichi_mpm_amd as tc_amd  # noqa: E402


def main(frames=10, res=64, frame_dt=2e-3, strength=40.0):
    """runs `frames` frames; returns what it prints: the particle count, the mean speed per frame, the ctx's host particle bytes at
    the end and how many of them the tensor calls added (0)"""
    import torch
    sim = tc_amd.create_simulation3("mpm")
    sim.initialize(dict(res=(res,) * 3, base_delta_t=1e-4, gravity=(0, -10, 0)))
    sim.set_levelset(tc_amd.LevelSet(friction=0.4).add_plane((0, 1, 0), d=-0.3))  # floor y = 0.3
    sim.add_particles(dict(type="sand", cube_lo=(res * 3 // 8,) * 3, cube_cells=res // 4, friction_angle=30))
    sim._ensure_ctx()
    host_bytes = lambda: int(sim._L.mpmhip_host_particle_bytes(sim._ctx))  # noqa: E731
    n = sim.get_num_particles()
    print("particles:", n)
    axis = torch.tensor([0.5, 0.5], device="cuda:%d" % sim.device)
    by_tensor_calls, mean_speed = 0, []
    for frame in range(frames):
        before = host_bytes()
        p = sim.get_particle_tensors(("x", "v"))
        mean_speed.append(float(p["v"].norm(dim=1).mean()))
        print("frame %d: mean speed %.4f" % (frame, mean_speed[-1]))
        r = p["x"][:, [0, 2]] - axis                                        # the swirl: a(x) = strength * (-r_z, 0, r_x)
        p["v"][:, 0] -= frame_dt * strength * r[:, 1]
        p["v"][:, 2] += frame_dt * strength * r[:, 0]
        sim.set_particle_tensors(dict(v=p["v"]))
        by_tensor_calls += host_bytes() - before
        sim.step(frame_dt)
    total = host_bytes()
    print("mpmhip_host_particle_bytes: %d (by the tensor calls: %d)" % (total, by_tensor_calls))
    out = dict(particles=n, mean_speed=mean_speed, host_particle_bytes=total, host_particle_bytes_of_the_tensor_calls=by_tensor_calls)
    sim.close()
    return out


if __name__ == '__main__':
    main(frames=int(sys.argv[1]) if len(sys.argv) > 1 else 10, res=int(sys.argv[2]) if len(sys.argv) > 2 else 64)
