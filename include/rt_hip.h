/*
 * rt_hip.h -- C-ABI of the MI355X (gfx950) per-pixel ray-trace hot path.
 *
 * Drop-in device path for the two reference renderers of
 * markrosoft/se-195-project-ray-tracer:
 *
 *   Whitted (raytracer3.0.06.no_rec.samp): rtw_* replace the OpenCL device
 *     path of openCLcode.cpp -- AllocateBuffers (:64-120), SetKernelArguments
 *     (:562-624), ExecuteKernel / clEnqueueNDRangeKernel (:537-560) and
 *     ReadKernelBuffer (:626-643) -- and compute what the CPU path
 *     Engine_Render (raytracer.cpp:301-530) computes, bit for bit.
 *   smallpt (smallptgpu-v1.6): spt_* replace ExecuteKernel (smallptGPU.cpp:617-640)
 *     and the buffer traffic of UpdateRenderingGPU (:642-782) / ReInit*GPU
 *     (:784-830), computing UpdateRenderingCPU's per-pixel result
 *     (smallptCPU.cpp:84-123: flipped colour/seed slot, running average, toInt).
 *   Queue tracer (Raytracer3.2.03): rtq_* replace raytracer_non_kernel
 *     (raytracer_non_OpenCL.c:285-449), the CPU twin its raytracer.c:756
 *     calls in place of run_openCL_kernel (:417-640), computing its uchar4
 *     frame bit for bit.
 *
 * Plain pointers and sizes only.  Every entry point returns RT_OK (0) or a
 * negative RT_ERR_* code; rt_last_error() describes the last failure of the
 * calling thread.  Struct layouts are byte-identical to the reference's.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_ERR_INVALID -1   /* bad argument (null pointer, size, row range) */
#define RT_ERR_HIP -2       /* HIP runtime failure (rt_last_error has the text) */
#define RT_ERR_NODEVICE -3  /* no gfx950 device visible */

typedef struct { float x, y, z; } rt_vec3;

/* raytracer.h:23-32 (Material :18-21, plane common.h:49-53) -- 96 bytes */
typedef struct {
    int32_t type;                 /* SPHERE = 1, PLANE = 2, BOX = 3 */
    int32_t m_Light;
    rt_vec3 m_Centre;
    float m_SqRadius, m_Radius, m_RRadius;
    rt_vec3 plane_N;
    float plane_D;
    float plane_cell[4];
    rt_vec3 m_Color;
    float m_Refl, m_Refr, m_Diff, m_Spec, m_RIndex;
} rt_primitive;

/* smallptgpu-v1.6/geom.h:43-47 -- 44 bytes */
typedef struct {
    float rad;
    rt_vec3 p, e, c;
    int32_t refl;                 /* DIFF = 0, SPEC = 1, REFR = 2 */
} rt_sphere;

/* smallptgpu-v1.6/camera.h:29-34 -- 60 bytes */
typedef struct {
    rt_vec3 orig, target;
    rt_vec3 dir, x, y;
} rt_camera;

/* Raytracer3.2.03 raytracer_non_OpenCL.c:42-44 float_4 */
typedef struct { float x, y, z, w; } rtq_float4;

/* Raytracer3.2.03 raytracer_non_OpenCL.c:67-81 Primitive_2 -- 96 bytes
 * (the C++ bool is_light is one byte). */
typedef struct {
    rtq_float4 m_color;
    float m_refl, m_diff, m_refr, m_refr_index, m_spec, dummy_3;
    int32_t type;                 /* PLANE = 0, SPHERE = 1 */
    uint8_t is_light;
    uint8_t pad_[3];
    rtq_float4 normal, center;
    float depth, radius, sq_radius, r_radius;
} rtq_primitive;

/* ------------------------------------------------------------ runtime */
const char *rt_last_error(void);
int rt_device_count(void);
/* Select the HIP device used by the calling thread's subsequent calls. */
int rt_set_device(int device);
/* Release the per-device buffers the blocking entry points cache. */
int rt_release(void);
/* Bytes of device memory the blocking entry points currently cache. */
size_t rt_cached_bytes(void);
/* Page-locked host memory (hipHostMalloc) for frames the host reads back
 * every pass -- the smallpt drop-in's `pixels` (smallptGPU.cpp:111, a plain
 * malloc there, read by ReadKernelBuffer :626 after every pass): its
 * device-to-host copy then runs at DMA speed instead of through a staging
 * buffer.  rt_host_free(NULL) is a no-op. */
int rt_host_alloc(size_t bytes, void **out);
int rt_host_free(void *p);

/* ------------------------------------------------------------ Whitted */
/* Blocking, host buffers.  Renders rows [row_begin,row_end) of the w x h
 * frame into xrgb (uint32 0x00RRGGBB, row-major), leaving other rows
 * untouched; the reference window is [20, h-70) (raytracer.cpp:281,307).
 * Requires 20 <= row_begin < row_end <= h (m_SY's recurrence starts at row 20).
 * counters (nullable, host, 4 x u64): traced rays, shadow rays,
 * Primitive_Intersect calls, total-internal-reflection events -- the same
 * quantities oracle/orw_render counts. */
int rtw_render(const rt_primitive *prims, int nprims, uint32_t *xrgb, int w, int h,
               int row_begin, int row_end, uint64_t *counters);

/* Asynchronous, device-resident.  d_prims: device copy of the primitive
 * array; d_xrgb: device frame (w*h); d_counters: device u64[4] accumulated
 * into (nullable); stream: hipStream_t (NULL = default stream).  Work is
 * ordered on `stream`: a large frame also runs on a library-owned second
 * stream, forked from `stream` and joined back to it by events before the
 * call's last operation. */
int rtw_render_async(const rt_primitive *d_prims, int nprims, uint32_t *d_xrgb, int w, int h,
                     int row_begin, int row_end, uint64_t *d_counters, void *stream);

/* The reference's own device kernel instead of its CPU path: raytrace_kernel
 * of raytracer3.0.06.no_rec.samp/openCLcode.cl:5-247 with openCLcode.h's
 * Engine_Raytrace (ExecuteKernel, openCLcode.cpp:537-560) -- rows
 * [20, min(530, h)) (openCLcode.cl:66-67), SX = WX1 + x*DX per pixel (:22-23),
 * 2x2 sub-samples (:66), a light hit adds the light's colour
 * (openCLcode.h:176-182), reflection child folded before the refraction child
 * (:199-233), x(256/4) scale (:238-240), the channels ORed into the pixel
 * (:245; the CPU path adds them), a shadow ray's occluders the primitives with
 * m_Light < 1 (openCLcode.h:235; the CPU path: == 0).  The OpenCL built-ins (sqrt, '/',
 * exp, pow) are computed as the CPU path's correctly rounded / glibc
 * functions.  Same counters as rtw_render.  Rows outside the window are not
 * written. */
int rtw_render_ocl(const rt_primitive *prims, int nprims, uint32_t *xrgb, int w, int h,
                   uint64_t *counters);
int rtw_render_ocl_async(const rt_primitive *d_prims, int nprims, uint32_t *d_xrgb, int w, int h,
                         uint64_t *d_counters, void *stream);

/* What colour does the tracer compute along this ray?  For each of the caller's
 * rays (d_rays: device memory, 6 floats per ray, o.xyz d.xyz, used as given:
 * the direction is NOT normalised) one sub-sample of Engine_Render
 * (raytracer.cpp:353-511) with o_Ray = refl_Ray = refr_Ray = that ray,
 * input_Rindex = 1 and the node arrays reset: the root Engine_Raytrace call,
 * the 62 children in breadth-first order (each traced iff its parent's refl /
 * refr > 0; a total-internal-reflection node's refraction child with the
 * refr_Ray variable as the earlier calls left it -- the last node before it
 * that wrote one, else the caller's own ray) and the back-accumulation.
 *   d_color[3r .. 3r+2]  tr_Color_{x,y,z}[0] after the back-accumulation.  The
 *                        reference adds both children's shares to it, traced
 *                        or not, so a channel is never -0.0;
 *   d_t[r]               tr_dist[0]: the root's distance, 1e6f on a miss
 *                        (nullable);
 *   d_id[r]              the root call's return: the primitive index or -1
 *                        (nullable).
 * The sub-sample grid, the x28 / x64 scale and the pack stay with the caller
 * (rtamd.scenes.whitted_camera_rays / whitted_pack restate the frame's).
 * flags: RTW_TRACE_OCL selects openCLcode.h / openCLcode.cl's semantics (a
 * light hit adds the light's colour, a shadow ray's occluders are the
 * primitives with m_Light < 1, the reflection child is folded first).
 * d_counters (nullable, device u64[4], accumulated into): rtw_render's four.
 * Every float is the reference's, bit for bit, for any ray and any primitive
 * floats; where the reference's value is a NaN, some NaN.
 *
 * Ordered on `stream` as rtw_render_async is -- serialised with the other
 * level-pass frames on the device, whose arena it shares -- but on that one
 * stream only.  The rays run in slabs of up to 18 M, one after the other
 * (RT_WHITTED_TRACE_SLAB=<rays>, rounded up to 64, forces small ones and
 * RT_WHITTED_QUEUE_CAP a small record pool: test hooks, the same bits).  NOT
 * promised to be graph-capturable: the arena may grow, and sizing the record
 * pool reads a host flag.  nrays == 0 is RT_OK and launches nothing.  The
 * outputs must not alias the inputs; an output that is not asked for is not
 * written.  RT_ERR_INVALID before any device work: a null d_prims, d_rays or
 * d_color; nprims outside 1..64; unknown flag bits; nrays above INT32_MAX. */
#define RTW_TRACE_OCL 0x1
int rtw_trace_async(const rt_primitive *d_prims, int nprims, const float *d_rays, size_t nrays, int flags,
                    float *d_color, float *d_t, int *d_id, uint64_t *d_counters, void *stream);
/* Blocking, host buffers; counters (nullable, host u64[4]) receives this
 * call's counts.  The device copies are the call's own allocation, freed
 * before it returns. */
int rtw_trace(const rt_primitive *prims, int nprims, const float *rays, size_t nrays, int flags,
              float *color, float *t, int *id, uint64_t *counters);

/* ------------------------------------------------------------ smallpt */
#define SPT_PATH_TRACING 0       /* RadiancePathTracing    geomfunc.h:167-338 */
#define SPT_DIRECT_LIGHTING 1    /* RadianceDirectLighting geomfunc.h:340-483 */
/* Flag OR-ed into `mode` of the device-resident entry points: with
 * d_counters, count only counters[0] (Intersect calls), [1] (IntersectP
 * calls) and [3] (samples) -- SURVEY §8(d)'s rays -- and leave counters[2]
 * (sphere tests) untouched.  The sphere-test count needs IntersectP's
 * early-exit position (geomfunc.h:94-110: the highest-index occluder), which
 * costs hierarchy scenes a longer shadow walk; the call counts do not. */
#define SPT_COUNT_RAYS 0x100
/* Flag OR-ed into `mode` of spt_scene_render_list_async with d_group_cost:
 * each listed group's entry receives the LONGEST of its tiles' wave times
 * (atomic max) instead of their sum -- the length of the group's slowest
 * pixel chain, the order key for the heavy-tile treatment (list such groups
 * first), where the sum is the load to balance. */
#define SPT_COST_MAX 0x200
/* Flag OR-ed into `mode` of spt_scene_render_list_async only: the caller
 * guarantees that d_groups is already a set (no repeats, every entry in
 * range -- rtamd.dist.ListGather checks its lists on the host), so the
 * per-call dedup pass (a stream-ordered scratch allocation, a fill, one
 * small kernel, the free) is skipped.  A list that breaks the promise may
 * render a group twice in one launch: results are then undefined. */
#define SPT_LIST_SET 0x800

/* Blocking, host buffers, whole frame.  Runs samples first_sample ..
 * first_sample+nsamples-1 of every pixel, exactly as nsamples successive
 * UpdateRenderingCPU passes with currentSample = first_sample, ...:
 *   colors  float[3*w*h]  Vec per pixel, slot (h-y-1)*w+x      (in/out)
 *   seeds   uint32[2*w*h] two MWC words per slot (h-y-1)*w+x    (in/out)
 *   pixels  uint32[w*h]   toInt(r) | toInt(g)<<8 | toInt(b)<<16 at y*w+x (out)
 * mode: SPT_PATH_TRACING or SPT_DIRECT_LIGHTING.  counters (nullable,
 * host, 4 x u64): Intersect calls, IntersectP calls, sphere tests, samples. */
int spt_render(const rt_sphere *spheres, unsigned nspheres, const rt_camera *camera,
               float *colors, uint32_t *seeds, uint32_t *pixels, int w, int h,
               int first_sample, int nsamples, int mode, uint64_t *counters);

/* Device-resident buffers, rows [row_begin,row_end) of the frame.  Buffers
 * are full-frame device arrays laid out as above; seeds are read from
 * d_seeds_in and the advanced state written to d_seeds_out (may alias).
 * camera is read on the host at call time (passed by value to the kernel).
 * Reads the sphere array back (synchronising `stream` once) to find or
 * prepare the device's cached scene -- prepared again only when the array's
 * contents change -- then launches asynchronously; use spt_scene_* to stay
 * fully asynchronous.  spt_render uses the same cache. */
int spt_render_async(const rt_sphere *d_spheres, unsigned nspheres, const rt_camera *camera,
                     float *d_colors, const uint32_t *d_seeds_in, uint32_t *d_seeds_out,
                     uint32_t *d_pixels, int w, int h, int row_begin, int row_end,
                     int first_sample, int nsamples, int mode, uint64_t *d_counters,
                     void *stream);

/* Prepared scene: uploads the sphere array once (device SoA of geometry,
 * materials and per-light records; for >= 256 spheres also the exact-culling
 * sphere hierarchy).  Reuse it across frames.
 *
 * Sphere fields may be any floats; no scene is rejected for its values.  As
 * in the reference (geomfunc.h:32-59) the radius counts only through rad *
 * rad -- a sphere of radius -2 is the sphere of radius 2 -- and a sphere whose
 * radius or centre is not finite is never hit.  A hierarchy scene keeps both
 * rules: boxes are taken from |rad|, and a sphere whose float box c -+ |rad|
 * is not finite widens no box, so its frames and query answers are the full
 * scan's, bit for bit.  A NaN accumulator (an infinite emitter channel times
 * a zero throughput) packs as the reference's x86-64 build packs it: the
 * float-to-int conversion gives INT_MIN. */
typedef struct spt_scene spt_scene;
int spt_scene_create(const rt_sphere *spheres, unsigned nspheres, spt_scene **out);
int spt_scene_destroy(spt_scene *scene);
/* A read-only description of a prepared scene and of the most recent launch
 * on it, for tests and tools: fills out[0 .. min(nout, SPT_INFO_WORDS)).
 * Host bookkeeping only -- no device work, no synchronisation; the launch
 * words are written by the thread that launches.  The scene's words:
 *   [0] kernel family: SPT_GEO_LDS (the scene staged in LDS, full scan),
 *       SPT_GEO_GLOBAL (full scan from global memory), SPT_GEO_BVH (binary
 *       hierarchy walked from global memory), SPT_GEO_WIDE (8-wide hierarchy
 *       in LDS).  (An SPT_GEO_LDS scene's launch runs the global-memory
 *       kernel where its block -- scene copy and per-wave areas, [16] -- would
 *       exceed a compute unit's LDS: the same bits either way.)
 *   [1] spheres   [2] lights (emitters)
 *   [3] spheres tested outside the hierarchy (|radius| > 64 x the median
 *       |radius|, NaN radii apart; <= 16)
 *   [4] binary hierarchy nodes   [5] 8-wide nodes   [6] 8-wide levels
 *   [7] the 8-wide tree's leaf size, 8, 12 or 16 (0: no 8-wide tree)
 *   [8] 1 if no sphere takes the refraction branch
 * The most recent launch's words (all 0 before the first):
 *   [9] launches so far   [10] waves per block   [11] blocks
 *   [12] lanes per pixel of the cooperative tier, 8, 4 or 2 (0: none)
 *   [13] cooperative (tier-1) tiles   [14] routed (tier-2) tiles
 *   [15] 1 if the two-query iteration ran   [16] dynamic LDS bytes per block */
#define SPT_GEO_LDS 0
#define SPT_GEO_GLOBAL 1
#define SPT_GEO_BVH 2
#define SPT_GEO_WIDE 3
#define SPT_INFO_WORDS 17
int spt_scene_info(const spt_scene *scene, int *out, int nout);

/* spt_render_async on a prepared scene: asynchronous on `stream`
 * (graph-capturable).  Hierarchy scenes (>= 256 spheres) learn a dispatch
 * order: the first launch of a (window, camera, nsamples, mode) key records
 * each tile group's wave time and queues a 32-KB-class read-back of it; once
 * that has landed, launches of the key dispatch the heaviest groups first
 * (one small upload).  Scheduling only -- results are identical; during
 * stream capture the learnt order is used but not updated.  A scene's order
 * is updated by the calling thread: render one scene from one host thread
 * at a time.  That thread may have launches of the scene in flight on
 * several streams at once: the library orders the scene's own state (the
 * learnt order and the work counters) across them -- a new order never
 * lands in a buffer a running launch dispatches from, a counter entry is
 * not handed out again while its launch runs -- without blocking the host
 * and without allocating.  The caller's buffers stay the caller's to order.
 * Hierarchy scenes give every launch one of 64 work-counter
 * entries; a launch captured into a graph keeps its entry for the graph's
 * life (the graph may be replayed at any time), so at most 64 captured
 * launches of one scene can exist -- the next capture fails RT_ERR_INVALID
 * until spt_scene_release_captures. */
int spt_scene_render_async(const spt_scene *scene, const rt_camera *camera, float *d_colors,
                           const uint32_t *d_seeds_in, uint32_t *d_seeds_out, uint32_t *d_pixels,
                           int w, int h, int row_begin, int row_end, int first_sample, int nsamples,
                           int mode, uint64_t *d_counters, void *stream);

/* Hands the work-counter entries held by captured launches of `scene` out
 * again.  Call it only once every graph captured from this scene's launches
 * has been destroyed (a replay after it could share an entry with a new
 * launch). */
int spt_scene_release_captures(const spt_scene *scene);

/* Replaces spheres [first, first + count) of a prepared scene with
 * spheres[0 .. count) (host memory) in place; the sphere count stays.  Any
 * field may change, to any float (spt_scene_create's contract: the radius
 * counts through rad * rad, a non-finite sphere is never hit; the refit takes
 * boxes from |rad| and leaves a sphere whose float box is not finite out of
 * every box).  The caller may change or free `spheres` as soon as the
 * call returns (it is copied into page-locked staging the scene keeps).
 * Device work is ordered on `stream` and nothing is synchronised: launches on
 * `stream` enqueued before the call render the old scene, launches enqueued
 * after it the new one.  (Launches on other streams need the caller's own
 * ordering, as for any buffer.)  The scene's device must be the current one;
 * update and render one scene from one host thread at a time.
 *
 * The host re-derives the light list, the light count and the no-refraction
 * flag by spt_scene_create's rules, so kernel selection follows the edited
 * scene.  A hierarchy scene is refitted on the device: the tree keeps its
 * topology -- the always / tree partition, the leaf size, the octant child
 * order, the 8-wide slots, the highest-index table and the escape links -- and
 * every box, margin and quantised child box is recomputed from the new
 * spheres with the builders' own expressions.  Culling is exact, so the frames
 * are those of a scene created from the edited array, bit for bit; the learnt
 * dispatch order and the work counters stay.  A tree refitted after large
 * changes, or many times, may walk slower than a fresh one (its splits and
 * its partition were chosen for the original spheres, and its leaves still
 * hold the spheres they were dealt then): spt_scene_regroup_async re-deals the
 * spheres into the tree on the device, stream-ordered; spt_scene_create
 * remains the remedy for splits and a partition that no longer fit.
 *
 * The first update of a scene builds what a refit needs (the topology, once
 * more on the host; device metadata; staging) and is as slow as a create; a
 * scene that is never updated pays nothing.  One path synchronises: when the
 * edit raises the number of emitters above what the scene's light records
 * have room for, the records are reallocated (stream and device are waited
 * for; spt_scene_update_info counts it).  Graphs captured from this scene's
 * launches before such a reallocation hold the old address: capture again.
 *
 * RT_ERR_INVALID, with the scene untouched: a null pointer, a range out of
 * bounds, a capturing stream, another current device. */
int spt_scene_update_async(spt_scene *scene, const rt_sphere *spheres, unsigned first, unsigned count,
                           void *stream);
/* Host bookkeeping of spt_scene_update_async, fills out[0 .. min(nout,
 * SPT_UPDATE_INFO_WORDS)): [0] updates so far  [1] hierarchy refits run
 * [2] light-record rebuilds  [3] synchronising reallocations  [4] bytes of
 * refit metadata on the device (topology, entry boxes, node boxes; 0 before
 * the first update and for a scene without a hierarchy). */
#define SPT_UPDATE_INFO_WORDS 5
int spt_scene_update_info(const spt_scene *scene, uint64_t *out, int nout);

/* Moves spheres [first, first + count) of a prepared scene from DEVICE memory:
 * d_geom holds four floats per sphere (p.x, p.y, p.z, rad; sphere first + i
 * takes entry i), on the scene's device, 16-byte aligned.  Only the centre and
 * the radius change.  Emission, colour and refl stay, and with them the light
 * list and the light count, the no-refraction flag, the kernel family, every
 * launch parameter and every address: the host derives nothing, so the call
 * copies nothing to or from the host, stages nothing, allocates nothing and
 * synchronises nothing once the scene is prepared (below).  Any floats, under
 * spt_scene_create's contract: the radius counts through rad * rad, a sphere
 * with a non-finite centre or radius is never hit, boxes are taken from
 * |rad|, and a sphere whose float box is not finite widens no box.
 *
 * After a move the scene is, bit for bit, the scene spt_scene_update_async
 * leaves from the same edited spheres: the AoS array, the SoA geometry, the
 * light record of a moved emitter and, for a hierarchy scene, the entries'
 * geometry and boxes and the refit of every node, margin and 8-wide child box
 * (three launches: a gather that reads d_geom, then the update's two refit
 * kernels).  d_geom is read by the call's own kernels only: the caller may
 * overwrite it in stream order right after the call.  Launches on `stream`
 * enqueued before the call see the old scene, launches after it the new one.
 * The library's host copy of the spheres does not follow a move;
 * spt_scene_read_spheres reads the current ones.
 *
 * spt_scene_move_prepare builds what a move relies on -- what the first
 * update builds (topology, device metadata), the light index array on the
 * device, and entry boxes that hold the whole scene (one whole-scene refit on
 * `stream`) -- or whichever of these an earlier update or regroup left
 * missing.  It may allocate and it waits for `stream`.  An uncaptured move of
 * an unprepared scene prepares it first.
 *
 * Capture: on a capturing stream a prepared scene's move is recorded (fixed
 * kernels, every argument by value); each replay moves the spheres to what
 * d_geom holds at that replay.  An unprepared scene fails RT_ERR_INVALID
 * there.  As for captured launches of the scene, an spt_scene_update_async
 * that later changes the light count or reallocates the light records leaves a
 * recorded move stale: capture again.  Covered by the tests: a graph of a
 * move and a render of a scene WITHOUT a hierarchy (fewer than 256 spheres);
 * a graph of a hierarchy scene's move alone, the frames after its replays
 * being ordinary launches.  Not covered, and to be avoided: replaying a
 * captured render of a hierarchy scene with an edit of any kind (update,
 * regroup, move) between capture and replay or recorded in the same graph --
 * such replays have skipped work and hung ("Captured
 * graphs across scene edits").
 *
 * RT_ERR_INVALID, with the scene untouched: a null scene or d_geom, a d_geom
 * that is not 16-byte aligned, a range out of bounds, another current device,
 * a capturing stream on an unprepared scene (move) or at all (prepare).
 * count == 0 returns RT_OK and launches nothing. */
int spt_scene_move_prepare(spt_scene *scene, void *stream);
int spt_scene_move_async(spt_scene *scene, const float *d_geom, unsigned first, unsigned count, void *stream);
/* Host bookkeeping of spt_scene_move_async, fills out[0 .. min(nout,
 * SPT_MOVE_INFO_WORDS)): [0] moves enqueued (count > 0)  [1] those recorded on
 * a capturing stream  [2] hierarchy refits they launched (the prepare's
 * whole-scene refit is not one).  Replays of a recorded move are not counted. */
#define SPT_MOVE_INFO_WORDS 3
int spt_scene_move_info(const spt_scene *scene, uint64_t *out, int nout);
/* Blocking (waits for the device), for tests and tools: the scene's spheres as
 * the device holds them, scene-many records into out[0 .. cap).  A `cap` below
 * the sphere count fails RT_ERR_INVALID. */
int spt_scene_read_spheres(const spt_scene *scene, rt_sphere *out, unsigned cap);

/* Re-deals the current spheres of a prepared scene into the frozen shape of
 * its hierarchy, on the device, and refits: top-down, the entries of every
 * inner binary node's range are stable-sorted along the node's split axis by
 * the total-order integer key of their centres (bits ^ (bits >> 31 ?
 * 0xffffffff : 0x80000000); no float is compared, a NaN has its place), and
 * the left child takes the lower part.  Frozen: the always / tree partition,
 * every node's entry range and axis, the octant layouts and their links, the
 * 8-wide slots and child words, the leaf size, the node counts, the LDS
 * layout and the kernel family -- so no launch parameter changes, nothing is
 * reallocated, graphs captured from this scene's launches stay valid and the
 * learnt dispatch order stays.  Changed: which sphere sits at which tree
 * position, and what follows from it (the entries' geometry, every box,
 * margin and quantised child box, the 8-wide highest-index table).  Culling
 * is exact, so frames, queries, radiance and pixel-list calls enqueued on
 * `stream` before the call and after it give the same bits; the later ones
 * walk tighter leaves.  When to regroup is the caller's decision (after an
 * animation has carried the spheres away from where the tree was built).
 *
 * Device work is ordered on `stream` and nothing is synchronised.  The first
 * regroup of a scene builds its metadata and scratch (and, for a scene never
 * updated, what the first spt_scene_update_async builds, which
 * spt_scene_update_info then reports); later calls allocate nothing.  A sort
 * over more than 256 entries ranks by counting, quadratic in the range: fine
 * for tens of thousands of spheres, not meant for millions.  A scene without a
 * hierarchy returns RT_OK and launches nothing.
 *
 * RT_ERR_INVALID, with the scene untouched: a null scene, a capturing stream,
 * another current device. */
int spt_scene_regroup_async(spt_scene *scene, void *stream);
/* Host bookkeeping of spt_scene_regroup_async, fills out[0 .. min(nout,
 * SPT_REGROUP_INFO_WORDS)): [0] regroups run  [1] levels of the binary tree
 * [2] levels sorted by passes of their own (those that hold a range above
 * 256 entries; the rest is sorted in LDS, a subtree per block)  [3] bytes
 * of regroup metadata and scratch on the device.  All 0 before the first
 * regroup and for a scene without a hierarchy. */
#define SPT_REGROUP_INFO_WORDS 4
int spt_scene_regroup_info(const spt_scene *scene, uint64_t *out, int nout);
/* Blocking (waits for the device), for tests and tools: the hierarchy as the
 * device holds it, five sections back to back in `out` -- the node records of
 * the eight octant layouts (two float4 each), the entries' geometry (float4:
 * centre, rad^2; tree entries, then the always entries), their sphere
 * indices, the 8-wide nodes (28 words each), the 8-wide highest-index table
 * (8 words per node) -- with their byte sizes in sizes[0..4] (all 0 for a
 * scene without a hierarchy).  out == NULL: the sizes only; a `cap` below
 * their sum fails RT_ERR_INVALID. */
int spt_scene_read_hierarchy(const spt_scene *scene, void *out, size_t cap, size_t sizes[5]);

/* spt_scene_render_async over an interleaved window: every pixel row y with
 * (y / 8) % ngroups == group, i.e. 8-row groups group, group + ngroups, ...
 * (0 <= group < ngroups).  The ngroups windows of a frame partition it; a
 * multi-GPU frame split this way gives each GPU the same mix of the image
 * (contiguous bands differ in cost with their content).  Same results per
 * pixel as any other window. */
int spt_scene_render_groups_async(const spt_scene *scene, const rt_camera *camera, float *d_colors,
                                  const uint32_t *d_seeds_in, uint32_t *d_seeds_out, uint32_t *d_pixels,
                                  int w, int h, int group, int ngroups, int first_sample, int nsamples,
                                  int mode, uint64_t *d_counters, void *stream);

/* Tile groups: group g is the 8x8-pixel tiles 4g .. 4g+3 of the frame in
 * row-major tile order (ceil(w/8) tiles per row) -- a 32x8 strip when
 * ceil(w/8) is a multiple of 4.  spt_group_count(w, h) = ceil(ceil(w/8) *
 * ceil(h/8) / 4) (or a negative RT_ERR_*). */
int spt_group_count(int w, int h);

/* spt_scene_render_async over an explicit set of tile groups: d_groups
 * (device, ngroups entries in [0, spt_group_count(w, h)); entries outside
 * are skipped; the list is taken as a set -- a repeated group renders once,
 * at the dispatch slot of one of its copies) in dispatch order -- the first
 * ones start first, so list the costliest first.  A multi-GPU frame split by per-rank lists
 * balanced on measured costs (rtamd.dist.balanced_partition).  d_group_cost
 * (nullable, device, spt_group_count(w, h) words; hierarchy scenes only,
 * left unchanged otherwise): each listed group's wave time in 100 MHz ticks
 * is ADDED to its entry (zero it first).  With full counters (d_counters
 * set, no SPT_COUNT_RAYS) a lane that finishes its pixel takes the next one
 * (pixel refill), so there the unit is a pixel: the entry receives the sum
 * of its pixels' durations, or with SPT_COST_MAX the longest one -- a lane
 * time, not a wave time.  No order is learnt on this path.
 * Same results per pixel as any other window. */
int spt_scene_render_list_async(const spt_scene *scene, const rt_camera *camera, float *d_colors,
                                const uint32_t *d_seeds_in, uint32_t *d_seeds_out, uint32_t *d_pixels,
                                int w, int h, const int *d_groups, int ngroups, int first_sample,
                                int nsamples, int mode, uint64_t *d_counters, unsigned *d_group_cost,
                                void *stream);

/* The accumulator of listed tile groups to / from a packed buffer of 768
 * floats per group (its four tiles in turn, 64 pixels each in row-major
 * order, r g b; pixels outside the frame pack as 0 and are not unpacked):
 * the exchange of a frame split by group lists (one all-gather of the packed
 * shares).  Exact copies, asynchronous on `stream`. */
int spt_groups_pack_async(const float *d_colors, int w, int h, const int *d_groups, int ngroups,
                          float *d_out, void *stream);
int spt_groups_unpack_async(float *d_colors, int w, int h, const int *d_groups, int ngroups,
                            const float *d_in, void *stream);

/* The toInt pack of UpdateRenderingCPU (smallptCPU.cpp:120-122, vec.h:62)
 * alone: d_pixels[y*w+x] for rows [row_begin,row_end) from the accumulator
 * slots (h-y-1)*w+x of d_colors -- the pixels a render call writes, rebuilt
 * from colours that arrived from other ranks (a row-band frame assembled by
 * one colour all-gather).  Asynchronous on `stream`. */
int spt_pack_pixels_async(const float *d_colors, uint32_t *d_pixels, int w, int h, int row_begin,
                          int row_end, void *stream);

/* ------------------------------------------------------------ smallpt, ray queries */
/* What does this ray hit?  Caller-supplied rays against a prepared scene's
 * current spheres, with the loops and hierarchy walks rendering uses.
 *
 * d_rays: device memory, 6 floats per ray (o.xyz, d.xyz), used as given: the
 * direction is NOT normalised, and a direction of any length is exact.
 * d_tmax: device memory, one float per ray -- maxt for ANY and OCCLUDER
 * (required); for NEAREST the initial bound, NULL meaning 1e20f, which is
 * Intersect.  d_t, d_id: device memory, one element per ray; they must not
 * alias the inputs.  NEAREST writes whichever of the two is given (at least
 * one); ANY and OCCLUDER write d_id, which they require, and never d_t.
 *
 * With d_i the float distance of SphereIntersect (geomfunc.h:32-59: its
 * operations in its order, unfused, correctly rounded square root; 0 = miss)
 * for sphere i, and the accepted set A = { i : d_i != 0 && d_i < bound }:
 *   NEAREST   d_id[r] = the i in A of smallest d_i, ties to the highest index,
 *             or -1; d_t[r] = that d_i, or on a miss the bound's own bits.
 *   ANY       d_id[r] = 1 if A is not empty, else 0 (IntersectP's answer).
 *   OCCLUDER  d_id[r] = the highest i in A (where IntersectP's descending
 *             loop returns), or -1.
 * These are the results of a full scan of all spheres, bit for bit, whichever
 * kernel family the scene runs.  Any float may stand anywhere: a ray with a
 * non-finite component hits nothing (the formula's own outcome), and a bound
 * that is <= EPS (0.01f) or NaN accepts nothing.
 *
 * Asynchronous on `stream`; allocates nothing, never synchronises and takes
 * no work-counter entry, so any number of calls may be captured into graphs.
 * Ordered after earlier spt_scene_update_async calls on the same stream: a
 * query enqueued after an update sees the edited spheres.  nrays == 0 is
 * RT_OK and launches nothing.  RT_ERR_INVALID: a null scene or d_rays, an
 * unknown kind, no output the kind writes, a missing d_tmax where required,
 * nrays above INT32_MAX, another current device.
 * RT_SPT_QUERY_BLOCKS=<n> (read at the call) caps the grid, for tests. */
#define SPT_QUERY_NEAREST  0  /* Intersect,  geomfunc.h:71-92 */
#define SPT_QUERY_ANY      1  /* IntersectP, geomfunc.h:94-110: occluded or not */
#define SPT_QUERY_OCCLUDER 2  /* IntersectP's exit position: the highest-index occluder */
int spt_scene_query_async(const spt_scene *scene, const float *d_rays, const float *d_tmax, size_t nrays,
                          int kind, float *d_t, int *d_id, void *stream);

/* ------------------------------------------------------------ smallpt, radiance queries */
/* What radiance arrives along this ray?  The reference's estimator on
 * caller-supplied rays against a prepared scene's current spheres, in the
 * kernel family the scene renders with.
 *
 * d_rays: device memory, 6 floats per ray (o.xyz, d.xyz), used as given and
 * NOT normalised, as for spt_scene_query_async.  d_seeds_in / d_seeds_out:
 * device memory, the ray's two MWC words (simplernd.h) at 2r and 2r + 1; the
 * two may be the same buffer.  d_radiance: device memory, 3 floats per ray,
 * the ray's running average: read and written when first_sample > 0, only
 * written when first_sample == 0; it must not alias the rays or the seeds.
 * mode: SPT_PATH_TRACING or SPT_DIRECT_LIGHTING, without flag bits.
 *
 * For ray r, with (s0, s1) read from d_seeds_in, for j = 0 .. nsamples - 1:
 *   R = RadiancePathTracing(spheres, n, &ray_r, &s0, &s1)   geomfunc.h:167-338
 *       (or RadianceDirectLighting, :340-483),
 *   current = first_sample + j,
 *   d_radiance[r] = current == 0 ? R : (d_radiance[r] * k1 + R) * k2 per
 *       component, k1 = (float)current, k2 = 1.f / (k1 + 1.f)
 *       (smallptCPU.cpp:110-118),
 * and (s0, s1) is then written to d_seeds_out: bit for bit what the
 * reference's functions return for that ray and state, whichever family the
 * scene runs.  No camera draw is taken: a caller who wants the reference's
 * pixel jitter draws it before the call.  A ray whose first Intersect misses
 * -- every ray with a non-finite component among them -- yields (0, 0, 0)
 * for that sample and draws nothing.  nsamples == 0 copies the seeds and
 * leaves d_radiance alone.
 *
 * Asynchronous on `stream`; allocates nothing, never synchronises and takes
 * no work-counter entry, so any number of calls may be captured into graphs.
 * Ordered after earlier spt_scene_update_async calls on the same stream.
 * nrays == 0 is RT_OK and launches nothing.  RT_ERR_INVALID: a null scene,
 * d_rays, d_seeds_in, d_seeds_out or d_radiance, a negative nsamples or
 * first_sample, an unknown mode or one carrying flag bits, nrays above
 * INT32_MAX, another current device.
 * RT_SPT_QUERY_BLOCKS=<n> (read at the call) caps the grid, for tests. */
int spt_scene_radiance_async(const spt_scene *scene, const float *d_rays, size_t nrays,
                             const uint32_t *d_seeds_in, uint32_t *d_seeds_out,
                             float *d_radiance, int first_sample, int nsamples, int mode,
                             void *stream);

/* ------------------------------------------------------------ smallpt, pixel lists */
/* Samples where the caller wants them: a list of pixels, each with its own
 * sample count, rendered into the frame buffers of the other entry points.
 *
 * d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h: the frame, as for
 * spt_scene_render_async (colours and seeds at slot (h-y-1)*w+x, d_pixels at
 * y*w+x; the two seed buffers may be one).  w * h must fit an int32.
 * d_list: device memory, nlist pixel indices p = y*w+x, the index d_pixels
 * uses.  An entry outside [0, w*h) is skipped, so -1 padding is legal.  The
 * caller guarantees that d_list is a set: no per-call check is made, and a
 * pixel listed twice is traced by two lanes that race on one RNG chain and
 * one accumulator -- results are then undefined (the SPT_LIST_SET promise,
 * which this entry point always takes).
 * d_take: nullable, device memory, nlist counts: the samples to add to entry
 * e's pixel; a negative count is taken as 0.  NULL: every entry takes
 * nsamples.  With d_take, nsamples must be 0.
 * d_done: nullable, device memory, w*h int32 at the colour slot: a fourth
 * plane of the accumulator holding the pixel's currentSample.  Given, a
 * pixel's samples are numbered d_done[slot] + j and d_done[slot] += take is
 * written back; first_sample must then be 0.  NULL: they are numbered
 * first_sample + j, as everywhere else.
 * mode: SPT_PATH_TRACING or SPT_DIRECT_LIGHTING, without flag bits.
 *
 * Per listed pixel with take t: (s0, s1) is read from d_seeds_in and, when
 * the first sample's number is > 0, the running average from d_colors; then
 * for j = 0 .. t-1 the two jitter values are drawn, the camera ray is built
 * exactly as UpdateRenderingCPU builds it (smallptCPU.cpp:84-105),
 * RadiancePathTracing or RadianceDirectLighting runs, and the result is
 * folded as smallptCPU.cpp:110-118 folds it; after the last sample the colour,
 * the advanced seeds (to d_seeds_out) and d_pixels[p] (the toInt pack) are
 * written.  An entry with t == 0 copies its two seed words to d_seeds_out and
 * writes nothing else.  Pixels that are not listed are not touched in any
 * buffer, d_seeds_out included.  Per pixel the result is what any other
 * window computes for that sample range, bit for bit, whichever kernel family
 * the scene runs: "pixel p after n samples" does not depend on what the
 * other pixels were given.
 *
 * Asynchronous on `stream`; allocates nothing, never synchronises, takes no
 * work-counter entry and keeps no per-launch state, so any number of calls
 * may be captured into graphs; learns no dispatch order.  Ordered after
 * earlier spt_scene_update_async calls on the same stream.  nlist == 0 is
 * RT_OK and launches nothing.  RT_ERR_INVALID: a null scene, camera, d_colors,
 * d_seeds_in, d_seeds_out, d_pixels or d_list; w or h < 1 (or w * h above
 * INT32_MAX); a negative nsamples or first_sample; d_take together with
 * nsamples > 0; d_done together with first_sample > 0; an unknown mode or one
 * carrying flag bits; nlist above INT32_MAX; another current device.
 * RT_SPT_QUERY_BLOCKS=<n> (read at the call) caps the grid, for tests. */
int spt_scene_render_pixels_async(const spt_scene *scene, const rt_camera *camera,
                                  float *d_colors, const uint32_t *d_seeds_in, uint32_t *d_seeds_out,
                                  uint32_t *d_pixels, int w, int h,
                                  const int32_t *d_list, const int32_t *d_take, size_t nlist, int nsamples,
                                  int32_t *d_done, int first_sample, int mode, void *stream);

/* The same call, keeping a second-moment plane beside the colour: what an
 * adaptive sampler needs to decide where the next samples go.
 *
 * d_m2: required, device memory, w*h floats at the colour slot (h-y-1)*w+x;
 * it must not alias the other buffers.  Everything
 * spt_scene_render_pixels_async specifies holds unchanged: colours, seeds,
 * d_pixels and d_done come out bit for bit as from that call with the same
 * arguments.  In addition, for a listed pixel with take t > 0 whose first
 * sample has number `base`, each sample j with radiance R (the value folded
 * into the colour) folds
 *     q  = (R.x*R.x + R.y*R.y) + R.z*R.z            (float, unfused)
 *     m2 = (base + j == 0) ? q : (m2*k1 + q)*k2     (the colour fold's k1, k2)
 * so d_m2[slot] is the running mean of |R|^2 as d_colors is the running mean
 * of R: read when base > 0, written together with the colour.  With the
 * stored colour c, m2 - |c|^2 is the summed per-channel variance of the
 * pixel's samples.  A sample whose camera ray is non-finite folds q = 0; a
 * take of 0, an entry outside the frame and an unlisted pixel leave
 * d_m2[slot] untouched; a non-finite R gives whatever the expressions give.
 *
 * Asynchronous, capturable and validated as spt_scene_render_pixels_async;
 * RT_ERR_INVALID also for a null d_m2.  RT_SPT_QUERY_BLOCKS applies. */
int spt_scene_render_pixels_stats_async(const spt_scene *scene, const rt_camera *camera,
                                        float *d_colors, const uint32_t *d_seeds_in, uint32_t *d_seeds_out,
                                        uint32_t *d_pixels, float *d_m2, int w, int h,
                                        const int32_t *d_list, const int32_t *d_take, size_t nlist, int nsamples,
                                        int32_t *d_done, int first_sample, int mode, void *stream);

/* ------------------------------------------------------------ smallpt, the sample plan */
/* The next pixel list of a frame, built on the device from its colours,
 * second moments and sample counts: "render until every pixel's relative
 * standard error is below tol, at most max_samples samples" is K x (plan,
 * render) enqueued back to back, or one graph.  No scene is involved.
 *
 * Per slot i, with n = d_done[i] and c its colour, in float, unfused:
 *   n < min_samples:  take = min_samples - n, e = +inf
 *   otherwise:        mean2 = (c.x*c.x + c.y*c.y) + c.z*c.z
 *                     var   = d_m2[i] - mean2;  var = var > 0 ? var : 0   (NaN -> 0)
 *                     e     = sqrtf(var / ((float)n * (mean2 + floor)))
 *                     take  = (e > tol && n < max_samples) ? min(step, max_samples - n) : 0
 * (a NaN e is not listed; the n/(n-1) factor is left out: min_samples guards
 * small n).  The pixels with take > 0 go to d_list[j] = y*w+x, d_take[j], in
 * 8 x 8 tile order -- ascending ((y>>3)*tiles_x + (x>>3))*64 + (y&7)*8 + (x&7),
 * tiles_x = (w+7)/8 -- entries of rank >= cap are dropped, and every position
 * from the number written up to cap gets d_list = -1, d_take = 0: the caller
 * passes nlist = cap to spt_scene_render_pixels*_async whatever was listed.
 * d_error: nullable, w*h floats at the slot: e.  d_totals: nullable, 2 words:
 * the pixels listed (before truncation) and the sum of their takes.
 * d_scratch: device memory of spt_frame_plan_scratch_bytes(w, h) bytes (0 for
 * a frame size that is not valid), 16-byte aligned, the call's alone until it
 * has run; its contents mean nothing to the caller.
 *
 * Three stream-ordered launches; asynchronous, allocates nothing, never
 * synchronises, keeps no state: any number of calls may be captured.
 * cap == 0 writes only d_error / d_totals.  RT_ERR_INVALID: a null d_colors,
 * d_m2, d_done, params or d_scratch, a null d_list or d_take unless cap == 0;
 * w or h < 1, or w*h above INT32_MAX; min_samples < 1, max_samples <
 * min_samples or step < 1; a NaN or negative tol or floor; cap above
 * INT32_MAX. */
typedef struct {
    int32_t min_samples, max_samples, step;
    float tol, floor;
} spt_plan_params;
size_t spt_frame_plan_scratch_bytes(int w, int h);
int spt_frame_plan_async(const float *d_colors, const float *d_m2, const int32_t *d_done, int w, int h,
                         const spt_plan_params *params, int32_t *d_list, int32_t *d_take, size_t cap,
                         float *d_error, uint64_t *d_totals, void *d_scratch, void *stream);

/* ------------------------------------------------------------ smallpt, several GPUs */
/* One frame tiled over the GPUs of a node in row bands:
 * band k owns the k-th contiguous chunk of the flipped colour / seed slots,
 * i.e. pixel rows [h - e_k, h - s_k) with B = ceil(h/ngpus), s_k = min(h, k*B),
 * e_k = min(h, (k+1)*B) -- equal bands (the last one shorter, or empty), so
 * one in-place all-gather of B rows per band assembles the frame.
 * Every pixel keeps its RNG words and accumulator on its band's device, so
 * rendering needs no exchange; samples of a pixel are never split.  One host
 * thread drives all devices (one stream each), as the reference's single
 * host thread drove its one OpenCL queue (smallptGPU.cpp:617-640,739-760).
 *
 * devices: ngpus device ordinals (NULL: 0..ngpus-1).  A device may repeat
 * (several bands on one GPU -- the same band/assemble code on one device).
 * Each band holds a full-frame colour / seed / pixel array on its device;
 * only its own rows are authoritative until spt_multi_gather_async. */
typedef struct spt_multi spt_multi;
int spt_multi_create(const rt_sphere *spheres, unsigned nspheres, int w, int h, const int *devices,
                     int ngpus, spt_multi **out);
int spt_multi_destroy(spt_multi *m);
/* Re-uploads the scene to every band's device (ReInitSceneGPU). */
int spt_multi_set_scene(spt_multi *m, const rt_sphere *spheres, unsigned nspheres);
/* spt_scene_update_async on every band's scene, each on its band's stream:
 * no band is re-prepared or waited for (but for the cases that call names). */
int spt_multi_update_scene(spt_multi *m, const rt_sphere *spheres, unsigned first, unsigned count);
/* spt_scene_regroup_async on every band's scene, each on its band's stream:
 * no band is re-prepared or waited for. */
int spt_multi_regroup_scene(spt_multi *m);
/* Pixel-row bounds: rows[k] .. rows[k+1] hold band k's rows in FLIPPED
 * order, i.e. band k renders pixel rows [h - rows[k+1], h - rows[k]).
 * rows: ngpus + 1 ints. */
int spt_multi_bands(const spt_multi *m, int *rows);
/* Host -> bands: each band's rows of seeds (2*w*h words, flipped slots) and,
 * when colors is not NULL, of the accumulator (3*w*h floats).  Blocking. */
int spt_multi_upload(spt_multi *m, const float *colors, const uint32_t *seeds);
/* Samples first_sample .. first_sample+nsamples-1 of every pixel, each band
 * on its own device, asynchronous.  counters: accumulate the four
 * spt_render counters (read with spt_multi_counters). */
int spt_multi_render_async(spt_multi *m, const rt_camera *camera, int first_sample, int nsamples,
                           int mode, int counters);
/* Assembles the whole HDR accumulator on every band's device and repacks
 * each device's RGBA8 frame from it (spt_pack_pixels_async).  Distinct
 * devices: one in-place ncclAllGather of the equal (padded) bands over xGMI
 * (the padding rows past h are never read); repeated devices or
 * RT_SPT_GATHER=peer: stream-ordered peer copies (RT_SPT_GATHER=rccl runs the
 * RCCL all-gather even for a single band).  Asynchronous. */
int spt_multi_gather_async(spt_multi *m);
/* Waits for every band's device work. */
int spt_multi_sync(spt_multi *m);
/* Bands -> host, blocking: each band's rows of colors / seeds / pixels
 * (each nullable) -- the assembled frame, no collective needed. */
int spt_multi_download(spt_multi *m, float *colors, uint32_t *seeds, uint32_t *pixels);
/* Band k's whole device frame -> host, blocking (after a gather: the
 * assembled frame as band k's device holds it).  Either pointer nullable. */
int spt_multi_read_frame(spt_multi *m, int k, float *colors, uint32_t *pixels);
/* Sums the per-band counters into out[4] (blocking) and zeroes them. */
int spt_multi_counters(spt_multi *m, uint64_t *out);
/* Band k's device frame and stream (after a gather: the whole frame). */
int spt_multi_band_buffers(const spt_multi *m, int k, int *device, float **d_colors, uint32_t **d_seeds,
                           uint32_t **d_pixels, void **stream);

/* spt_render over several GPUs (SURVEY.md §8(b) "spt_render(..., ngpus)"):
 * the same contract and results as spt_render, the frame tiled in row bands
 * over devices[0..ngpus-1] (NULL: 0..ngpus-1), host buffers assembled band
 * by band.  Blocking.  The band context (per band: scene, buffers, stream)
 * is kept across calls: the same devices and frame size reuse it, a changed
 * sphere array re-prepares only the scenes; rt_release frees it. */
int spt_render_multi(const rt_sphere *spheres, unsigned nspheres, const rt_camera *camera,
                     float *colors, uint32_t *seeds, uint32_t *pixels, int w, int h,
                     int first_sample, int nsamples, int mode, uint64_t *counters,
                     const int *devices, int ngpus);
/* Diagnostics of spt_render_multi's cached context: out[0] = band contexts
 * built, out[1] = scene preparations (both since the process started). */
int spt_multi_cache_info(uint64_t *out);

/* ------------------------------------------------------------ queue tracer (3.2.03) */
/* Blocking, host buffers, whole frame: raytracer_non_kernel(pixels, w, h,
 * prims, nprims) (raytracer_non_OpenCL.c:285-449).  pixels: w*h uchar_4
 * (r, g, b, 0) row-major -- as uint32, r | g<<8 | b<<16.  counters (nullable,
 * host, 4 x u64): rays traced (raytrace calls), shadow rays, intersect calls,
 * undefined-behaviour events.  The last counts what the reference leaves
 * undefined and this library defines as "no child rays": a ray at depth < 5
 * that hits nothing (the reference then reads primitives[-1], :373) or hits a
 * light with m_refl or m_refr > 0 (point_intersect is uninitialised, :197).
 * Neither occurs in the reference scene (scene.c:53-97). */
int rtq_render(const rtq_primitive *prims, int nprims, uint32_t *pixels, int w, int h,
               uint64_t *counters);
/* Asynchronous, device-resident: rows [row_begin,row_end) of the w x h frame
 * (0 <= row_begin < row_end <= h; other rows untouched) into d_pixels (w*h);
 * d_counters: device u64[4] accumulated into (nullable).  Ordered on
 * `stream` as rtw_render_async (a frame of several slabs also uses the
 * library's second stream, forked and joined by events). */
int rtq_render_async(const rtq_primitive *d_prims, int nprims, uint32_t *d_pixels, int w, int h,
                     int row_begin, int row_end, uint64_t *d_counters, void *stream);

/* What colour does the tracer compute along these rays?  d_rays: device
 * memory, 6 floats per ray (o.xyz d.xyz), used as given: the direction is NOT
 * normalised.  A queue-tracer pixel is not a sum of per-ray colours: it is
 * one sequential float chain over every node of all its primaries' trees in
 * queue order, `acc` carried from one sub-sample into the next
 * (raytracer_non_OpenCL.c:314-368).  So the rays come in chains: chain c is
 * rays [c group, (c + 1) group), group = 1..64, nrays a multiple of group.
 * Per chain (:309-434): acc = 0; for each of its rays in order a Ray with
 * that origin and direction, weight 1, depth 0, origin_primitive -1, type
 * ORIGIN, r_index 1 and transparency (1, 1, 1) is pushed and the FIFO drained
 * -- raytrace (:179-281) per popped ray, its term added to acc by its type
 * (:351-368), the reflected, then the refracted child pushed while depth < 5
 * (:370-432).  group = 1 is the colour along one ray; group = 9 over a
 * frame's camera rays is the frame.
 *   d_color[3c .. 3c+2]  acc after chain c's last ray has drained;
 *   d_t[r]               the root raytrace call's *a_dist for ray r, 1e7f on a
 *                        miss (nullable);
 *   d_id[r]              its return: the primitive index or -1 (nullable).
 * The sub-sample grid, the x28 scale, the clamp and the uchar4 pack stay with
 * the caller (rtamd.scenes.queue_camera_rays / queue_pack restate the
 * frame's).  d_counters (nullable, device u64[4], accumulated into):
 * rtq_render's four.  Undefined behaviour is defined as for frames: a ray at
 * depth < 5 that hits nothing, or hits a light with m_refl or m_refr > 0,
 * queues no children and is counted in counters[3]; a caller's ray that
 * leaves the scene has a zero term and d_id -1.  Every float is the
 * reference's, bit for bit, for any ray and any primitive floats; where the
 * reference's value is a NaN, some NaN.
 *
 * Ordered on `stream` as rtq_render_async is -- serialised with the other
 * level-pass frames on the device, whose arena it shares -- but on that one
 * stream only.  The chains run in slabs of whole chains, at most 6 M rays
 * each, one after the other (RT_QUEUE_TRACE_SLAB=<rays>, rounded up to whole
 * chains and to 64 chains, forces small ones; RT_QUEUE_POOL_CAP and
 * RT_QUEUE_EXACT_ALL apply as to frames: test hooks, the same bits).  A trace
 * of N rays caches no more device memory than a frame of N trees.  NOT
 * promised to be graph-capturable: the arena may grow, and sizing the record
 * pool reads a host flag.  nrays == 0 is RT_OK and launches nothing.  The
 * outputs must not alias the inputs; an output that is not asked for is not
 * written.  RT_ERR_INVALID before any device work: a null d_prims, d_rays or
 * d_color; nprims outside 1..64; group outside 1..64; nrays not a multiple of
 * group; nrays above INT32_MAX. */
int rtq_trace_async(const rtq_primitive *d_prims, int nprims, const float *d_rays, size_t nrays, int group,
                    float *d_color, float *d_t, int *d_id, uint64_t *d_counters, void *stream);
/* Blocking, host buffers (color: 3 floats per chain); counters (nullable,
 * host u64[4]) receives this call's counts.  The device copies are the call's
 * own allocation, freed before it returns. */
int rtq_trace(const rtq_primitive *prims, int nprims, const float *rays, size_t nrays, int group,
              float *color, float *t, int *id, uint64_t *counters);

/* ------------------------------------------------------------ level-pass tracers, ray queries */
/* What does this ray hit, and is this point shadowed?  Caller-supplied rays
 * against the primitives of the Whitted tracer (raytracer3.0.06) or of the
 * queue tracer (Raytracer3.2.03), with the nearest-hit and shadow loops their
 * frames are rendered with.
 *
 * A prepared scene holds at most 64 primitives (the references allocate 50).
 * The creators take a HOST array and return when the scene is ready; the
 * array is free again then.  *_prims_set_async replaces the whole primitive
 * array from DEVICE memory (as rtw_render_async / rtq_render_async take it):
 * nprims may change, and so may which primitives are lights or occluders.
 * rtp_scene_destroy waits for the device; NULL is a no-op.
 *
 * d_rays: device memory, 6 floats per ray (o.xyz, d.xyz), used as given: the
 * direction is NOT normalised.  Any float may stand anywhere: the answers are
 * whatever the reference's own loop yields for those floats, NaN and
 * infinities included.  The outputs are device memory, one element per ray,
 * and must not alias the inputs.
 *
 * NEAREST: the reference's nearest-hit loop -- Whitted: raytracer.cpp:39-49
 * over Primitive_Intersect (scene.cpp:125-190), far = 1e6f; queue tracer:
 * raytracer_non_OpenCL.c:181-193, far = 1e7f -- i.e. the smallest distance
 * strictly below far, ties to the lowest primitive index:
 *   d_id[r]      the primitive index, or -1 on a miss;
 *   d_t[r]       the distance, bit for bit, or on a miss the tracer's far;
 *   d_result[r]  1 for a hit from outside (HIT), -1 for a hit from inside a
 *                sphere (INPRIM), 0 for a miss -- for both tracers (the queue
 *                reference's own variable would still hold its initial 1).
 * Each of the three is nullable; at least one must be given.  d_tmax
 * (nullable, one float per ray): a hit is reported only when its distance is
 * < d_tmax[r], strictly; far still applies (the bound is min(tmax, far)), and
 * a NaN bound accepts nothing.  That is what the reference's loop started at
 * the bound returns: a candidate's distance does not depend on the distance
 * to beat.
 *
 * SHADOW / OCCLUDER: the references' shadow loop (raytracer.cpp:76-110,
 * raytracer_non_OpenCL.c:224-241).  The occluders -- Whitted: the primitives
 * with m_Light == 0; queue tracer: those with !is_light -- are visited in
 * index order, each tested with the distance to beat set to d_tmax[r]
 * (required; no far applies):
 *   SHADOW    d_id[r] = 1 if any occluder is nearer than d_tmax[r], else 0;
 *   OCCLUDER  d_id[r] = the primitive index where the reference's loop
 *             breaks (the first such occluder in index order), or -1.
 * Both require d_id and never write d_t or d_result.
 *
 * Every call is asynchronous on `stream`, allocates nothing, never
 * synchronises and keeps no per-launch state, so any number of calls may be
 * captured into graphs.  A query enqueued after a *_prims_set_async on the
 * same stream sees the new primitives (other streams need the caller's own
 * ordering, as for any buffer); a captured set reads d_prims at every replay.
 * nrays == 0 is RT_OK and launches nothing.  RT_ERR_INVALID, with nothing
 * launched: a null scene, d_rays, prims or out; an unknown kind; no output the
 * kind writes; a missing d_tmax where required; nrays above INT32_MAX; nprims
 * outside 1..64; a set through the other tracer's entry point; a create while
 * the library's stream is capturing; another current device than the scene's.
 * The checks that need no device come first.
 * RT_PRIMS_QUERY_BLOCKS=<n> (read at the call) caps the grid and
 * RT_PRIMS_QUERY_RAYS=1|2 picks NEAREST's rays per lane, for tests and tools:
 * the same bits either way. */
typedef struct rtp_scene rtp_scene;
int rtw_prims_create(const rt_primitive *prims, int nprims, rtp_scene **out);
int rtq_prims_create(const rtq_primitive *prims, int nprims, rtp_scene **out);
int rtp_scene_destroy(rtp_scene *scene);
int rtw_prims_set_async(rtp_scene *scene, const rt_primitive *d_prims, int nprims, void *stream);
int rtq_prims_set_async(rtp_scene *scene, const rtq_primitive *d_prims, int nprims, void *stream);

#define RTP_QUERY_NEAREST  0  /* the nearest hit */
#define RTP_QUERY_SHADOW   1  /* shadowed or not */
#define RTP_QUERY_OCCLUDER 2  /* the shadow loop's exit: the first occluder in index order */
int rtp_query_async(const rtp_scene *scene, const float *d_rays, const float *d_tmax, size_t nrays, int kind,
                    float *d_t, int *d_id, int *d_result, void *stream);

/* Host helper: AllocateBuffers' seed fill (smallptGPU.cpp:105-110) --
 * srand(seed); seeds[i] = max(rand(), 2) for i < n, with the host libc's
 * rand() (glibc on the reference's Linux build). */
void spt_seed_fill(uint32_t *seeds, size_t n, unsigned seed);

#ifdef __cplusplus
}
#endif
#endif
