/*
 * oracle/ref/whitted_ocl_ref_driver.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference's OpenCL kernel (raytracer3.0.06.no_rec.samp/openCLcode.cl with
 * openCLcode.h), included in place and compiled as host C++ through
 * opencl_as_host.h, into oracle/_ref/libref_whitted_scene.so.  The reference's
 * text sits in a namespace of its own: it defines an Engine_Raytrace, a
 * Primitive and a Ray that differ from raytracer.cpp's, which the same library
 * holds.  ref_whitted_render_ocl runs raytrace_kernel once per work-item of the
 * w x h frame, as the reference's host code enqueues it; the kernel writes rows
 * [20, min(530, h)) and leaves the others alone.  What the pin assumes about
 * the OpenCL built-ins: see opencl_as_host.h.
 */
#include "opencl_as_host.h"

namespace ref_ocl {
#include "openCLcode.cl"
}

extern "C" int ref_ocl_sizeof_primitive(void) { return (int)sizeof(ref_ocl::Primitive); }

extern "C" void ref_whitted_render_ocl(const void *prims, int n, unsigned int *dest, int w, int h)
{
    ref_ocl::Primitive *p = (ref_ocl::Primitive *)prims;
    for (int gid = 0; gid < w * h; gid++) {
        ref_ocl_gid = gid;
        ref_ocl::raytrace_kernel(h, w, (int *)dest, p, n);
    }
}
