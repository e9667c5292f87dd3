/*
 * oracle/ref/whitted_ref_driver.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * Links the reference's own raytracer3.0.06.no_rec.samp/raytracer.cpp,
 * scene.cpp and surface.cpp (compiled unmodified, where they lie) into
 * oracle/_ref/libref_whitted_scene.so, so the C restatement in
 * oracle/whitted_oracle.c can be checked against them:
 *   - Scene_InitScene / Primitive_Intersect / Primitive_GetNormal, one call
 *     at a time;
 *   - ref_whitted_render: Engine_InitRender + Engine_Render (which call
 *     Engine_Raytrace) on the caller's primitives at any frame size -- the
 *     whole-frame pin of orw_render.
 * raytracer.cpp includes "windows.h" and "winbase.h" and uses nothing from
 * them: the build puts oracle/ref/win_stub, two empty headers of this
 * repository's own, first on the include path.  The engine's state is global
 * and it is single-threaded: one frame at a time.
 * The OpenCL kernel's twin, ref_whitted_render_ocl, is in
 * whitted_ocl_ref_driver.cpp.
 */
#include <string.h>
#include "common.h"
#include "raytracer.h"
#include "scene.h"

extern "C" int ref_whitted_scene(Primitive *out, int cap)
{
    Scene_InitScene();
    int n = m_Scene->m_Primitives;
    if (cap < n) return -1;
    memcpy(out, m_Scene->m_Primitive, sizeof(Primitive) * n);
    return n;
}

extern "C" int ref_primitive_intersect(Primitive *p, const float ray[6], float *dist)
{
    Ray r;
    r.m_Origin.x = ray[0]; r.m_Origin.y = ray[1]; r.m_Origin.z = ray[2];
    r.m_Direction.x = ray[3]; r.m_Direction.y = ray[4]; r.m_Direction.z = ray[5];
    return Primitive_Intersect(p, &r, dist);
}

extern "C" void ref_primitive_normal(const Primitive *p, const float pos[3], float out[3])
{
    vector3 q, n;
    q.x = pos[0]; q.y = pos[1]; q.z = pos[2];
    Primitive_GetNormal(&n, *p, q);
    out[0] = n.x; out[1] = n.y; out[2] = n.z;
}

extern "C" int ref_sizeof_primitive(void) { return (int)sizeof(Primitive); }

/* testapp.cpp's launch sequence with the scene replaced by the caller's
 * array: writes rows [20, h - 70) of dest (w * h pixels), nothing else. */
extern "C" void ref_whitted_render(Primitive *prims, int n, Pixel *dest, int w, int h)
{
    Scene *saved = m_Scene;
    Engine_Constructor();
    m_Scene->m_Primitive = prims;
    m_Scene->m_Primitives = n;
    TracedRays_init();
    Engine_SetTarget(dest, w, h);
    Engine_InitRender();
    Engine_Render();
    free(m_Scene);
    m_Scene = saved;
}
