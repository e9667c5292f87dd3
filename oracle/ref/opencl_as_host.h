/*
 * oracle/ref/opencl_as_host.h -- TEST INFRASTRUCTURE ONLY.
 *
 * Lets the reference's OpenCL C translation unit (openCLcode.cl, which
 * includes openCLcode.h) compile as host C++, unmodified and where it lies:
 * whitted_ocl_ref_driver.cpp includes this header and then the .cl file.
 *
 *   - the kernel and address-space qualifiers mean nothing on the host;
 *   - get_global_id(0) reads the work-item index the driver sets before each
 *     call of raytrace_kernel;
 *   - the built-ins sqrt, exp and pow on float are taken as glibc's float
 *     functions sqrtf, expf and powf.  THIS IS AN ASSUMPTION of the pin, the
 *     same one oracle/whitted_oracle.c (orw_render_ocl) states: an OpenCL
 *     device may round exp and pow differently (the standard allows a few
 *     ulp), so the pin says "the kernel's program text with correctly rounded
 *     sqrt and glibc expf / powf", not "what some OpenCL device printed".
 *     Without the mapping C++ would evaluate pow(float, 20) in double.
 */
#ifndef RT_ORACLE_OPENCL_AS_HOST_H
#define RT_ORACLE_OPENCL_AS_HOST_H

#include <math.h>

#define __kernel
#define kernel
#define __global
#define global

static int ref_ocl_gid;                  /* the work-item raytrace_kernel runs as */
#define get_global_id(dim) (ref_ocl_gid)

#define sqrt sqrtf
#define exp  expf
#define pow  powf

#endif
