// spt_move.h -- the gather of spt_scene_move_async: a geometry-only edit of a
// prepared smallpt scene whose source is device memory (four floats per
// sphere: p.x, p.y, p.z, rad).  It stands where refit_gather stands in an
// update; refit_nodes and refit_wide (spt_refit.h) follow it unchanged, and
// every value is formed by spt_refit.h's expressions, so a move leaves the
// bytes spt_scene_update_async leaves from the same edited spheres.
//
// The source rule.  spt_refit.h's ordering holds: no launch reads what another
// workgroup of the same launch wrote.  refit_gather reads the AoS array, which
// the update's copy filled earlier on the stream.  Here the AoS array is
// written by this launch (the lane of sphere first + t stores rad and p of its
// record), so no lane reads those fields: a lane that needs a moved sphere --
// its own, a hierarchy entry's, a light record's -- reads d_geom[id - first],
// which no lane writes.  What a move does not change (emission, colour, refl;
// the entries and light records of spheres outside the range) is not read and
// not written either: the colour | rad record and the light's colour | rad
// record get their fourth float alone.
//
// What a move relies on (spt_scene_move_prepare): the entry boxes hold the
// whole scene, and the light index array is on the device.
#ifndef SPT_MOVE_H
#define SPT_MOVE_H

#include "spt_refit.h"

#if defined(__HIPCC__)
namespace sptrefit {

// One lane per moved sphere, per hierarchy entry and per light record.
//   t < count:     sphere first + t <- geom[t]: rad and p of its AoS record, its
//                  SoA geo record, the rad of its colour record;
//   t < nb + na:   entry t, if its sphere lies in [first, first + count)
//                  -> geo (p, rad * rad) and, for a tree entry, its float box;
//   t < nlights:   light record t, if lights[t] lies in the range -> its geo
//                  record and the rad of its colour record.
__global__ void __launch_bounds__(256) move_gather(DevRefit v, const float4 *__restrict__ geom, int first, int count,
                                                   const int *__restrict__ lights, int nlights)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < count) {
        const int i = first + t;
        const float4 g = geom[t];
        float *q = (float *)(v.spheres + i);             // rt_sphere: rad, p.xyz, e, c, refl (4-byte aligned)
        q[0] = g.w; q[1] = g.x; q[2] = g.y; q[3] = g.z;
        v.soa[i] = make_float4(g.x, g.y, g.z, g.w * g.w);
        ((float *)(v.soa + 2 * (size_t)v.n + i))[3] = g.w;
    }
    if (v.nodes && t < v.nb + v.na) {
        const int i = v.ids[t];
        if ((unsigned)(i - first) < (unsigned)count) {
            const float4 g = geom[i - first];
            v.geo[t] = make_float4(g.x, g.y, g.z, g.w * g.w);
            if (t < v.nb) {
                float lo[3], hi[3];
                sphere_box(g.w, g.x, g.y, g.z, lo, hi);
                for (int k = 0; k < 3; k++) {
                    v.box[(size_t)k * v.nb + t] = lo[k];
                    v.box[(size_t)(3 + k) * v.nb + t] = hi[k];
                }
            }
        }
    }
    if (t < nlights) {
        const int i = lights[t];
        if ((unsigned)(i - first) < (unsigned)count) {
            const float4 g = geom[i - first];
            float4 *gl = v.soa + 3 * (size_t)v.n + 3 * (size_t)t;
            gl[0] = make_float4(g.x, g.y, g.z, g.w * g.w);
            ((float *)(gl + 1))[3] = g.w;
        }
    }
}

}  // namespace sptrefit
#endif  // __HIPCC__

#endif
