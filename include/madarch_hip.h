/* madarch_hip.h -- C ABI of libmadarch_hip.so, the MI355X (gfx950) back end
 * that replaces the OpenGL/GLSL dispatch of Madarch.Renderers.
 *
 * Every entry point below stands for one public operation of the reference
 * package `Madarch.Renderers` (madarch/madarch-renderers.ads:21-97) or for an
 * output of `Madarch.Scenes.Compile` (madarch/madarch-scenes.ads:47-76); the
 * reference file:line each one replaces is cited next to it.  An Ada body of
 * Madarch.Renderers binds these with `pragma Import (C, ...)` (see
 * INTEGRATION.md and ada/).
 *
 * Conventions (mirroring the reference):
 *  - plain pointers and sizes only; the library copies everything on call and
 *    keeps no caller pointer;
 *  - every function returns an int32 status, 0 = ok; the text of the last
 *    error of the calling thread is returned by mdh_last_error();
 *  - a handle is NOT thread safe (the reference is single threaded and calls
 *    Make_Current on every entry, madarch-renderers.adb:170,304);
 *  - primitives and lights are 1-based (Ada `Positive`), materials 0-based
 *    (`Materials.Id`, madarch-renderers.adb:349-367);
 *  - GL.Types.Single = float, GL.Types.Int = int32_t, Singles.Vector3 = 3
 *    contiguous floats, Singles.Matrix3 = 9 floats passed COLUMN-major;
 *  - entity blobs use the std140 element layout the reference computes in
 *    GPU_Types (support/gpu_types-structs.adb:23-38): vec3 aligned to 16,
 *    float/int aligned to 4, fields in declared component order.
 */
#ifndef MADARCH_HIP_H
#define MADARCH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdh_renderer mdh_renderer; /* opaque; = access Renderer_Internal (renderers.ads:109-145) */

/* status codes; the Ada body raises Program_Error / Constraint_Error from them */
enum {
   MDH_OK = 0,
   MDH_E_INVALID = 1,          /* bad argument (null pointer, negative size, ...)            */
   MDH_E_PROBE_MISMATCH = 2,   /* Program_Error "Probe_Count should match grid dimensions."
                                  (madarch-renderers.adb:63-65)                               */
   MDH_E_UNSUPPORTED_KIND = 3, /* primitive/light kind that is not a built-in one             */
   MDH_E_INDEX = 4,            /* Constraint_Error: index out of the declared range           */
   MDH_E_DEVICE = 5,           /* a HIP call failed (text in mdh_last_error)                  */
   MDH_E_NO_DEVICE = 6,        /* no gfx950 device visible: the library never falls back to
                                  the CPU                                                     */
   MDH_E_STATE = 7,            /* call not valid in this state (e.g. partitioning disabled)   */
   MDH_E_COMM = 8              /* librccl missing, or an RCCL call failed (text in mdh_last_error) */
};

/* = Madarch.Values.Value_Kind order (madarch-values.ads:8) */
typedef enum { MDH_VEC3 = 0, MDH_FLOAT = 1, MDH_INT = 2 } mdh_kind;

/* = Madarch.Components.Component (name, kind)  (madarch-components.ads) */
typedef struct {
   const char *name;
   int32_t kind; /* mdh_kind */
} mdh_component;

/* One primitive or light kind with its declared maximum:
 * Scenes.Primitive_Count / Light_Count (madarch-scenes.ads:15-23).  Built-in
 * names: "Sphere", "Plane", "Box", "Triangle" (madarch-primitives-*.ads),
 * "PointLight", "SpotLight" (madarch-lights-*.ads).
 *
 * Any other primitive name is a USER-DEFINED kind (Primitives.Create,
 * madarch-primitives.ads:24-30): its Distance, Normal and Material expressions --
 * the Exprs trees the reference turns into GLSL text (Exprs.To_GLSL,
 * madarch-exprs.adb:325-711) -- arrive as three MDH_X programs (below) that the
 * kernels interpret.  Built-in kinds leave the program fields NULL / 0.
 *
 * Any other LIGHT name is a user-defined light kind (Lights.Create,
 * madarch-lights.ads:20-24) with two programs in the same fields:
 *   dist_code   = Sample (l, pos, normal, dir, dist) -> vec3 radiance in R0, R1, R2
 *   normal_code = Position (l)                        -> vec3 in R0, R1, R2
 * wrapped as the generated sample_<Light> is (madarch-scenes.adb:497-549):
 * dir = Position (l) - pos; dist = length (dir); dir /= dist; return Sample (...). */
typedef struct {
   const char *name;
   int32_t max_count;
   int32_t n_components;
   const mdh_component *components;
   const int32_t *dist_code;     /* Distance (prim, x) -> float in R0            */
   int32_t dist_len;
   const int32_t *normal_code;   /* Normal (prim, x)   -> vec3 in R0, R1, R2     */
   int32_t normal_len;
   const int32_t *material_code; /* Material (prim)    -> int (raw bits) in R0   */
   int32_t material_len;
} mdh_kind_decl;

/* ---- MDH_X: the register program a user-defined kind's expressions compile to.
 *
 * 64 registers R0..R63 of 32 raw bits per ray; a program is a straight line of
 * int32 words, one instruction per word (two for MDH_X_LIT and MDH_X_SEL):
 *     word = op | dst << 8 | a << 16 | b << 24
 * Vector expressions are lowered by the front end to scalar instructions in the
 * order the GLSL contract of DESIGN.md section 5 fixes: a vec3 lives in three
 * registers, dot = (x x' + y y') + z z', dot2 (v) = dot (v, v), length = sqrt (dot2),
 * normalize = v / length component by component, cross = (ay bz - az by, az bx - ax bz,
 * ax by - ay bx), clamp (x, l, u) = min (max (x, l), u), Min (A, B, C) = min (min (A, B), C)
 * (madarch-exprs.adb:154-155); If_Then_Else evaluates both sides and selects (the
 * expressions have no side effects); Let_In binds registers.  Float literals are
 * rounded through Single'Image like every literal of the generated GLSL
 * (madarch-exprs.adb:330-336); E ** n with a literal integer n = 2..16 is repeated
 * multiplication, squaring from the most significant bit of n ((x^2)^2 x for n = 5).  Arithmetic is IEEE fp32, one operation per
 * instruction, division and square root correctly rounded.
 *
 * At the IEEE edges (tests/mdhx_cases.py holds every evaluator to these, bit for bit):
 *   - ADD SUB MUL DIV DIVF SQRT FLOOR are the IEEE 754 operations, round to nearest even, with
 *     gradual underflow, overflow to infinity and the signed zeros of the standard (sqrt (-0) = -0,
 *     x - x = +0, floor (-0) = -0).  A NaN result's sign and payload are UNSPECIFIED (0/0 is
 *     0xFFC00000 on x86 and 0x7FC00000 on gfx950): only its being a NaN is defined.  Every other
 *     result is defined on all its 32 bits.
 *   - MIN / MAX are minNum / maxNum: a NaN operand is ignored, two NaNs give a NaN; -0 is ordered
 *     below +0 in either operand order (min (+0, -0) = min (-0, +0) = -0, max = +0), as
 *     v_min_f32 / v_max_f32 do.
 *   - LT GT LE GE are 0 when an operand is a NaN; -0 equals +0.
 *   - SEL takes b when a != 0: a NaN condition takes b, -0 (and +0) take c.
 *   - SIGN of a NaN and of either zero is +0.  NEG and ABS act on the sign bit alone.
 *   - ITOF reads the register's bits as int32 and rounds once, to nearest even (2^24 + 1 -> 2^24,
 *     INT_MAX -> 2^31).
 *   - POW (x, y): NaN for x < 0 or a NaN x; 0 for x = +-0 whatever y is (pow (0, 0) = 0,
 *     pow (0, -1) = 0); NaN for a NaN y otherwise; for x = +inf: inf, 1 or 0 as y > 0, = 0, < 0;
 *     1 for x = 1 (also with y = +-inf); else 2^z with z = y log2 (x) in fp32: +inf for z >= 128,
 *     0 for z < -126 (results below the normal range are flushed), and within
 *     1.2e-6 max (1, |z|) relative of the exact power in between.
 *   - SIN COS TAN of +-inf and of a NaN are NaN; ATAN (+-inf) = +-pi/2, of a NaN NaN.  Beyond
 *     |x| ~ 1e4 the reduction of SIN COS TAN loses accuracy, from |x| >= 1e9 pi/2 on there is none.
 *     ACOS and ASIN are NaN for |x| > 1 and for a NaN. */
enum {
   MDH_X_LIT = 0,    /* R[dst] = the next word (raw bits)                          */
   MDH_X_MOV = 1,    /* R[dst] = R[a]                                              */
   MDH_X_COMP = 2,   /* R[dst] = float a of the instance: components in declaration
                        order, a vec3 takes 3 floats, float / int 1 (raw bits)     */
   MDH_X_POINT = 3,  /* R[dst] = argument float a.  Primitive programs: a = 0..2, the point.
                        Light Sample: 0..2 pos, 3..5 normal, 6..8 dir, 9 dist          */
   MDH_X_ADD = 4, MDH_X_SUB = 5, MDH_X_MUL = 6,
   MDH_X_DIV = 7,    /* true division: components of vector "/"                    */
   MDH_X_DIVF = 8,   /* Float "/" Float: true division in the render passes; L + R in
                        Eval_Distance_To when MDH_OPT_ADA_EVAL_DIV is set, as
                        Madarch.Values."/" computes it (madarch-values.adb:112)     */
   MDH_X_NEG = 9, MDH_X_ABS = 10, MDH_X_FLOOR = 11,
   MDH_X_SIGN = 12,  /* 1, -1 or 0 (GLSL sign)                                     */
   MDH_X_MIN = 13, MDH_X_MAX = 14, MDH_X_SQRT = 15,
   MDH_X_POW = 16,   /* the fp32 pow of the shading path (oracle/orc_math.h)       */
   MDH_X_LT = 17, MDH_X_GT = 18, MDH_X_LE = 19, MDH_X_GE = 20, /* 1.0f or 0.0f    */
   MDH_X_SEL = 21,   /* R[dst] = R[a] != 0 ? R[b] : R[c], c = low byte of the next word */
   MDH_X_ITOF = 22,  /* To_Float: R[dst] = (float) (int) R[a]                      */
   MDH_X_ACOS = 23,  /* the fp32 acos of the shading path                           */
   MDH_X_SIN = 24, MDH_X_COS = 25, MDH_X_TAN = 26, MDH_X_ASIN = 27, MDH_X_ATAN = 28,
                     /* explicit fp32 algorithms (oracle/orc_math.h), a few 1e-7 absolute */
   MDH_X_OPS = 29
};
#define MDH_X_REGS 64
#define MDH_X_MAX_WORDS 4096 /* per program */

/* = Scenes.Partitioning_Settings (madarch-scenes.ads:30-41) */
typedef struct {
   int32_t enable;
   int32_t index_count;
   int32_t border_behavior; /* 0 Clamp, 1 Fallback (scenes.ads:28) */
   int32_t grid_dimensions[3];
   float grid_spacing[3];
   float grid_offset[3];
} mdh_partitioning;

/* = Renderers.Probe_Settings (madarch-renderers.ads:23-29) */
typedef struct {
   int32_t radiance_resolution;
   int32_t irradiance_resolution;
   int32_t probe_count[2];
   int32_t grid_dimensions[3];
   float grid_spacing[3];
} mdh_probe_settings;

/* = Renderers.Volumetrics_Settings (madarch-renderers.ads:33-41) */
typedef struct {
   int32_t enabled;
   int32_t visibility_resolution[3];
   float visibility_step_size;
   int32_t scattering_resolution[2];
   float scattering_step_size;
} mdh_volumetrics;

/* = the arguments of Scenes.Compile (madarch-scenes.ads:47-53) */
typedef struct {
   int32_t n_prim_kinds;
   const mdh_kind_decl *prim_kinds;
   int32_t n_light_kinds;
   const mdh_kind_decl *light_kinds;
   mdh_partitioning partitioning;
   float max_dist;
   int32_t loop_strategy; /* 0 Split, 1 Unify (scenes.ads:45); same results, kept for the record */
} mdh_scene_desc;

/* ---- options: switches the reference fixes at shader-compile time (the M_*
 * macros of madarch-renderers.adb:109-143) or that the headless build adds ---- */
enum {
   /* atlas storage: 0 = RGB8 as the reference (render_passes.adb:94), 1 = fp32 */
   MDH_OPT_ATLAS_FORMAT = 0,
   /* screen pass content: 0 = full pixel_color_probes as draw_screen.glsl;
    * 1 = BASELINE config 1 (primary ray only, colour 0.5 n + 0.5, no tonemap);
    * 2 = BASELINE config 2 (direct PBR + AO, irradiance = 0, no indirect specular) */
   MDH_OPT_SCREEN_MODE = 1,
   /* M_AMBIENT_OCCLUSION_STEPS of the screen pass (default 3, renderers.adb:140) */
   MDH_OPT_AO_STEPS = 2,
   /* 1 = also write the primary-ray geometry buffer (hit index, t, steps) */
   MDH_OPT_GBUFFER = 3,
   /* image/probe sharding for one-process-per-GPU runs: this renderer draws the
    * screen tiles and probe slices of `rank` out of `world` (default 0 / 1).  mdh_comm_init sets
    * both; setting them by hand is for callers that bring their own exchange (mdh_frame_*) */
   MDH_OPT_RANK = 4,
   MDH_OPT_WORLD = 5,
   /* 1 = record HIP events around every pass (read with mdh_pass_time) */
   MDH_OPT_TIMING = 6,
   /* Eval_Distance_To arithmetic: 1 = reproduce Madarch.Values."/" on floats
    * (L + R, madarch-values.adb:112) as the Ada evaluator does; 0 = GLSL "/" */
   MDH_OPT_ADA_EVAL_DIV = 7,
   /* how mdh_render schedules consecutive frames (madarch-renderers.adb:302-321;
    * the results are those of the serial order in every case):
    *   0 = strictly one pass after the other;
    *   1 = the probe passes of a frame overlap the screen pass of the frame before
    *       it (second HIP stream, two atlas sets);
    *   2 (default) = also the screen passes of consecutive frames overlap (third
    *       stream, two framebuffers).
    * Sharded renderers keep frames in flight the same way (mdh_frame_begin / _probe_pass / _end);
    * renderers on a caller-supplied stream run serially. */
   MDH_OPT_FRAME_OVERLAP = 8,
   /* user-defined kinds: 1 (default) = the MDH_X programs are compiled into the
    * kernels with hiprtc the first time a pass runs (about two seconds per kernel,
    * cached per process), the analogue of the reference's runtime shader
    * compilation; 0 = the kernels interpret the programs (no compilation, ~60x
    * slower).  Same results bit for bit.  If hiprtc cannot build a scene the
    * renderer falls back to 0 by itself and mdh_last_error says why. */
   MDH_OPT_JIT = 9,
   /* sharded renderers (MDH_OPT_WORLD > 1): 1 (default) = the irradiance pass updates ALL
    * probes on every rank from the gathered radiance atlas instead of its own slice (the pass
    * is one workgroup per probe and far from filling a GPU: the same time, and the second
    * exchange of the frame is not needed); 0 = own slice only, to be exchanged. */
   MDH_OPT_IRRADIANCE_ALL = 10,
   /* where the window's RGBA8 pixels (mdh_swap_buffers) are made: 1 = every screen pass also stores them
    * straight into pinned host memory, over PCIe, beside its float store, and mdh_swap_buffers has nothing
    * to convert or copy; 0 = mdh_swap_buffers converts and copies the framebuffer itself; 2 (default) = 0
    * until the first mdh_swap_buffers, 1 from then on (a renderer that never swaps pays nothing). */
   MDH_OPT_WINDOW = 11,
   /* M_COMPUTE_INDIRECT_SPECULAR of the screen pass (madarch-renderers.adb:138 fixes it at 2; the macro selects
    * among four bodies at glsl/render_probes.glsl:264-272):
    *   0 = no indirect specular;
    *   1 = sample_radiance_with_specular (render_probes.glsl:71-136): the reflection's hit position lit by the
    *       radiance atlases of the eight cage probes of the SHADED point, weighted by soft shadows and trilinearly;
    *   2 (default) = sample_radiance_no_specular (:138-209): the best-facing visible cage probe of the reflection's
    *       hit, plus that point's direct specular (M_ADD_INDIRECT_SPECULAR = 1);
    *   3 = compute_indirect_specular (:211-244): the reflection's hit shaded in full (direct light + irradiance).
    * textureLod on the single-level atlases is level 0 in every mode. */
   MDH_OPT_INDIRECT_SPECULAR = 12,
   /* Temporal blending of the irradiance atlas -- NOT in the reference, off by default (SURVEY.md section 8f-4 lists
    * it as a deviation): the irradiance pass stores mix (fresh, previous, h) with h = value / 1000 (0 .. 999), `previous`
    * being the texel the atlas held before the pass, as stored (RGB8: its 8-bit levels).  0 = the reference. */
   MDH_OPT_HYSTERESIS_PERMILLE = 13,
   /* Scheduling only, no effect on any texel: 1 (default) = the radiance pass records every probe ray's primary-march
    * length and the next frame's pass takes the rays sorted by it (a wavefront pays the longest march among its 64
    * rays); 0 = rays in probe order. */
   MDH_OPT_RADIANCE_ORDER = 14,
   /* Scheduling only, no effect on any pixel: 1 (default) = a screen pass records how long every 8x8 tile's wavefront
    * took, and later passes start the tiles in that order, slowest first (a pass ends with its slowest wavefront: in
    * image order the passes of the reference's scenes spend 15 - 45 % of their time waiting for a few late, long
    * tiles); re-sorted after camera moves and geometry edits; 0 = tiles in image order. */
   MDH_OPT_SCREEN_ORDER = 15,
   /* READ-ONLY: 0 = this library computes the oracle's bits (DESIGN.md "numerics contract": the only kind that ships);
    * 1 = the labelled experiment build (`make -C madarch_amd/csrc fast`: hardware sqrt / rcp / log / exp, fused
    * multiply-adds, the irradiance fold in four partial sums), which holds BASELINE.json's 1e-4 tolerance at best.
    * Setting it to anything but the build's own value is refused. */
   MDH_OPT_NUMERICS = 16,
   /* 1 = a mip chain for the radiance atlas (default 0 = the reference's behaviour).  The reference asks
      textureLod for level 1 (mode 2, render_probes.glsl:197) and for mix (0, radiance_lods, 2 roughness)
      (mode 1, render_probes.glsl:84-86,131; probe_utils.glsl:17) of an atlas it allocates with ONE level
      (render_passes.adb:113): every tap reads level 0.  With the switch on, each screen pass first builds
      levels 1 .. radiance_lods of the radiance atlas it reads (2x2 box filter of the level below,
      ((a + b) + (c + d)) / 4 per channel in fp32, stored in the atlas's format) and the two taps read
      them as GL_LINEAR_MIPMAP_LINEAR would.  Needs a power-of-two radiance resolution
      (MDH_E_INVALID otherwise).  Levels can be read back: mdh_read_texture (MDH_TEX_RADIANCE_MIP0 + l). */
   MDH_OPT_RADIANCE_MIPS = 17,
   /* Scheduling only, no effect on any pixel: a screen launch whose tiles, as two or four wavefronts each (8x4 or 4x4
    * pixels: 32 or 16 of a wavefront's 64 lanes), stay within `value` wavefronts is launched that way -- a launch that
    * leaves the chip's wavefront slots empty (a small window) lasts as long as its slowest
    * wavefront, which then marches for a quarter of the tile only, and the tile's work runs on four SIMDs (whole frames only: a
    * rank's scattered tiles of a sharded frame measured no faster).  Default 2560
    * (half the slots of an MI355X at five wavefronts per SIMD); 0 = every tile one wavefront.  Launches of 2 048 tiles and
    * more (MDH_OPT_SCREEN_ORDER's) are never split. */
   MDH_OPT_SCREEN_SPLIT = 18,
   /* Where the kernels read a scene's geometry from -- no effect on any result.  A scene table that fits a workgroup's LDS
    * beside the kernels' own rows (every scene of the reference's first three examples) is staged there whole: residency 0.
    * A larger one (about 860 triangles and up: the obj_mesh example's 1000) keeps its geometry and material ids in device
    * memory, read through L2, and only the header, lights, materials and decode table in LDS: residency 1.  Reading the
    * option gives the residency of the scene as committed (pending edits are committed first).  Setting 1 FORCES residency 1
    * for a scene that would fit (tests and A/B runs; MDH_E_INVALID at the next commit for scenes with user-defined kinds,
    * which always live in LDS); setting 0 returns to the choice by size. */
   MDH_OPT_TABLE_RESIDENCY = 19,
   /* 1 = the triangles of the scene are walked through a bounding-volume hierarchy instead of being scanned one by one
    * (default 0) -- no effect on any result: a subtree is skipped only where no triangle in it can lower the running
    * minimum, so every pass keeps the bits of the scan ("A BVH over the triangles").  The library
    * builds the hierarchy when the scene is committed and rebuilds it when a Triangle instance or their count changed;
    * the scene then runs in global residency (MDH_OPT_TABLE_RESIDENCY reads 1).  For scenes without a space partition,
    * without user-defined kinds and with at most one Triangle kind: MDH_E_STATE otherwise; other values MDH_E_INVALID.
    * A scene that declares no triangles accepts it and nothing changes. */
   MDH_OPT_TRIANGLE_BVH = 20,
   /* 1 (default) = probe rays are not marched again while the scene's geometry stands still -- no effect on any texel.
    * A probe ray starts at a fixed probe in a fixed direction: whether and where it hits, the nearest primitive there, its
    * step count, the first step of the hit point's shadow and visibility rays and the visibility of its eight cage probes
    * follow from the geometry alone.  The first radiance pass over geometry that did not change since the pass before
    * writes them to a 16-byte record per ray; later passes read the records and compute only what lights, materials and
    * the irradiance atlas change (direct light with its shadow rays, the eight taps), from the same values with the same
    * operations.  Set_Primitive, Add_Primitive, Update_Partitioning and every option or slice change that a march depends
    * on end it: the next pass marches, the one after records again.  The brute-force and room-census kernels replay; scenes
    * with a space partition, user-defined kinds or global residency keep marching ("Exact work
    * elimination", item 11).  0 = march every pass; the records are dropped.  mdh_radiance_replay_stats counts the passes. */
   MDH_OPT_RADIANCE_REPLAY = 21,
   /* 1 = the screen pass's marches are not run again while camera and geometry stand still -- no effect on any pixel; 0
    * (default) = marched every pass.  A pixel's primary hit, its reflection ray's hit, the nearest primitive at both, the
    * first step and the eight cage-visibility bits of both shaded points and the occlusion term follow from the camera ray,
    * the geometry and the probe grid alone.  The first screen pass over an unchanged camera and scene writes them to a
    * 32-byte record per pixel; later passes read the records and compute only what lights, materials and the atlases
    * change (direct light with its shadow rays, the taps, the combine, volumetrics), from the same values with the same
    * operations: framebuffer, window pixels, geometry buffer and atlases keep every bit.  A camera setter with a new
    * value, Set_Primitive, Add_Primitive, Update_Partitioning, a material in use that goes below the reflection's roughness threshold
    * and every option that a screen march or the pixels' places depend on end it: the next pass marches, the one after
    * records again.  The fixed mode (MDH_OPT_SCREEN_MODE 0, MDH_OPT_INDIRECT_SPECULAR 0 or 2 without mips) of scenes
    * without a space partition, user-defined kinds or global residency replays; everything
    * else keeps marching ("Exact work elimination", item 12).  0 drops the records.
    * mdh_screen_replay_stats counts the passes. */
   MDH_OPT_SCREEN_REPLAY = 22,
   /* 1 (default) = a frame's radiance and irradiance passes are not launched once the probe atlases have stopped changing
    * -- no effect on any texel or pixel; 0 = launched in every frame.  Both passes are deterministic in the bits they read:
    * when a pass has stored the irradiance bits it was given and nothing else it reads has changed, every later pass
    * stores them again.  Every tracked irradiance pass counts the texels it stores with other bits than the set it read
    * and hands the count to the host through pinned memory; mdh_frame_begin reads what has arrived and never waits.  After
    * MDH_SETTLE_PASSES = 16 consecutive unchanged passes (all atlas sets then hold the same bits) frames rotate through
    * the sets, record their events and run every other pass as before, without the probe passes.  Every entry point counts
    * as an edit that ends this -- the next frame launches its passes -- except mdh_render and the mdh_frame_* calls,
    * mdh_finish, read-backs and getters, pass times and statistics, the camera setters, mdh_swap_buffers and the options
    * TIMING, SCREEN_ORDER, SCREEN_SPLIT, SCREEN_REPLAY, GBUFFER, WINDOW, AO_STEPS, INDIRECT_SPECULAR and this one (a light
    * set to the value it has is an edit too).  Single rank and MDH_OPT_SCREEN_MODE 0 only: a renderer with a communicator,
    * a peer exchange or MDH_OPT_WORLD > 1 launches every pass.  With MDH_OPT_TIMING a settled pass is still counted; its
    * time is the few microseconds between its two events.  0 forgets the run.  mdh_probe_settle_stats counts (DESIGN.md
    * section 4, "Exact work elimination", item 13). */
   MDH_OPT_PROBE_SETTLE = 23,
   /* the device-array ray queries (mdh_raycast_device, ..): a wavefront takes new rays from the launch's counter when at
    * least this many of its 64 lanes are idle (or none is busy).  1 .. 64, anything else MDH_E_INVALID; 64 = lock step, rounds of
    * 64 consecutive rays, the schedule of the host-array queries.  Whatever the value, every ray has the same bits.  The
    * default is the measured one ("Ray queries").  No pass reads it: setting it ends no replay and
    * no settle run. */
   MDH_OPT_RAY_STREAM_REFILL = 24,
   /* ... and the workgroups of 256 threads such a query may launch: 0 (default) = as many as the device holds at once (or
    * fewer, for a small batch), k > 0 = at most k -- room for the frames in flight beside a large batch.  Any number
    * serves every ray.  Negative: MDH_E_INVALID.  No pass reads it either. */
   MDH_OPT_RAY_STREAM_GROUPS = 25,
   /* an adaptive path-traced frame (mdh_path_frame_begin_adaptive): 1 = a round compacts the pixels still running, so that
    * their lanes fill whole wavefronts; 0 (default, the measured one: DESIGN.md section 4, "An adaptive path-traced frame") = a
    * retired pixel keeps its lane and idles.  Both values give every pixel the same bits.  No pass reads it: setting it
    * ends no replay and no settle run. */
   MDH_OPT_PATH_FRAME_COMPACT = 26
};

/* passes of Renderers.Render (madarch-renderers.adb:302-321) */
enum {
   MDH_PASS_RADIANCE = 0,   /* compute_probe_radiance.glsl        */
   MDH_PASS_IRRADIANCE = 1, /* update_probe_irradiance.glsl       */
   MDH_PASS_VISIBILITY = 2, /* compute_frustrum_visibility.glsl   */
   MDH_PASS_SCATTERING = 3, /* accumulate_scattering.glsl         */
   MDH_PASS_SCREEN = 4,     /* draw_screen.glsl                   */
   MDH_PASS_EXCHANGE = 5,   /* no pass of the reference: the all-gather of a sharded frame's atlas slices
                               (mdh_frame_exchange), timed like a pass (mdh_pass_time)                     */
   MDH_PASS_COUNT = 6
};

/* atlases / textures of the renderer (texture units 0-3, renderers.adb:239-279) */
enum { MDH_TEX_RADIANCE = 0, MDH_TEX_IRRADIANCE = 1, MDH_TEX_VISIBILITY = 2, MDH_TEX_SCATTERING = 3 };
#define MDH_TEX_RADIANCE_MIP0 16 /* mdh_read_texture only: + l = level l >= 1 of the radiance atlas (MDH_OPT_RADIANCE_MIPS) */

/* Renderers.Create (madarch-renderers.adb:91-300) together with Scenes.Compile
 * (madarch-scenes.adb:1378-1421).  `width`/`height` replace the window size
 * (Windows.Open; the build is headless).  `device` is the HIP device ordinal
 * (one process per GPU: pass LOCAL_RANK).  SURVEY.md section 8(b) sketches this argument as
 * `n_devices`; with one process per GPU -- the execution model of this build -- a renderer owns ONE
 * device, and the N-device frame is formed by the renderers of N processes joining a communicator
 * (mdh_comm_init below): `n_devices` is that call's `world`. */
int32_t mdh_create(int32_t width, int32_t height, const mdh_scene_desc *scene,
                   const mdh_probe_settings *probes, const mdh_volumetrics *volumetrics,
                   int32_t device, mdh_renderer **out);

/* the reference never frees a Renderer; explicit release is new and harmless */
int32_t mdh_destroy(mdh_renderer *r);

int32_t mdh_set_option(mdh_renderer *r, int32_t option, int32_t value);
int32_t mdh_get_option(mdh_renderer *r, int32_t option, int32_t *value);

/* Renderers.Set_Material (madarch-renderers.adb:349-367); id is 0-based */
int32_t mdh_set_material(mdh_renderer *r, int32_t id0, const float albedo[3], float metallic,
                         float roughness);
/* Renderers.Add_Material (madarch-renderers.adb:369-377) */
int32_t mdh_add_material(mdh_renderer *r, const float albedo[3], float metallic, float roughness,
                         int32_t *out_id0);

/* Renderers.Set_Primitive (madarch-renderers.adb:379-398); index1 is 1-based */
int32_t mdh_set_primitive(mdh_renderer *r, int32_t kind_ix, int32_t index1, const void *std140_blob,
                          int32_t nbytes);
/* Renderers.Add_Primitive (madarch-renderers.adb:435-456) */
int32_t mdh_add_primitive(mdh_renderer *r, int32_t kind_ix, const void *std140_blob, int32_t nbytes,
                          int32_t *out_count);
/* Renderers.Set_Light (madarch-renderers.adb:458-483): also sets the kind's
 * count and total_light_count to index1, as the reference does */
int32_t mdh_set_light(mdh_renderer *r, int32_t index1, int32_t light_kind_ix, const void *std140_blob,
                      int32_t nbytes);

/* Renderers.Set_Camera_Position / Set_Camera_Orientation (renderers.adb:485-497) */
int32_t mdh_set_camera_position(mdh_renderer *r, const float p[3]);
int32_t mdh_set_camera_orientation(mdh_renderer *r, const float m_colmajor[9]);

/* Renderers.Update_Partitioning (madarch-renderers.adb:757-775);
 * method: 0 CPU_Best, 1 CPU_Fast, 2 GPU_Fast (renderers.ads:93).  All three builders run on
 * the device; the call enqueues the build and returns -- frames in flight keep the table they
 * were launched with, everything launched afterwards uses the new one. */
int32_t mdh_update_partitioning(mdh_renderer *r, int32_t method);

/* Renderers.Render (madarch-renderers.adb:302-321): enqueues all passes of one
 * frame on the renderer's stream.  mdh_finish waits for them. */
int32_t mdh_render(mdh_renderer *r);
/* one pass only (for one-process-per-GPU runs that exchange atlas slices
 * between the passes, see DESIGN.md "Multi-GPU") */
int32_t mdh_render_pass(mdh_renderer *r, int32_t pass);
/* Render in three steps, for callers that put work of their own between the
 * passes: mdh_frame_begin, mdh_frame_probe_pass(MDH_PASS_RADIANCE), [exchange],
 * mdh_frame_probe_pass(MDH_PASS_IRRADIANCE), [exchange], mdh_frame_end (volumetric
 * passes + screen pass).  mdh_render is exactly that sequence without the exchanges,
 * and frames opened this way are kept in flight the same way (MDH_OPT_FRAME_OVERLAP).
 * While a frame is open the atlas reads, writes and device pointers refer to the
 * atlas set that frame is producing, and the caller's device work on it must be
 * ordered on the stream mdh_probe_stream names. */
int32_t mdh_frame_begin(mdh_renderer *r);
int32_t mdh_frame_probe_pass(mdh_renderer *r, int32_t pass);
/* the exchange step of an open frame of a renderer that has a communicator (mdh_comm_init): all-gather of
 * the ranks' slices of atlas `tex` (MDH_TEX_RADIANCE / MDH_TEX_IRRADIANCE), in place on the open frame's atlas
 * set, enqueued on the probe stream.  Without a communicator: nothing (MDH_OK). */
int32_t mdh_frame_exchange(mdh_renderer *r, int32_t tex);
int32_t mdh_frame_end(mdh_renderer *r);
int32_t mdh_finish(mdh_renderer *r);

/* ---- one frame on the N GPUs of a node: one process (and one renderer) per GPU.
 *
 * The reference draws a frame with ONE call on one GPU (Renderers.Render, madarch-renderers.adb:302-321).
 * SURVEY.md section 8(b)/(e) asks for the same call to draw it on N: every process creates its renderer on its
 * own device, the processes join a communicator (RCCL over xGMI; librccl is opened on first use, the
 * library does not link it), and from then on mdh_render of every rank IS one frame of the sharded schedule:
 *    radiance pass for the rank's probe slice -> all-gather of the slices, in place on the probe-major atlas,
 *    on the probe stream -> irradiance pass (all probes on every rank, MDH_OPT_IRRADIANCE_ALL; own slice +
 *    a second all-gather otherwise) -> volumetric passes (replicated) -> screen pass for the 8x8 tiles
 *    t = rank (mod world).
 * Frames stay in flight exactly as on one GPU (MDH_OPT_FRAME_OVERLAP).  No caller-side collective, no other
 * runtime in the process: a host written in Ada or C needs only these calls and a way to hand 128 bytes from
 * rank 0 to the others (a file, a pipe, an environment variable).
 *
 *   mdh_comm_unique_id   rank 0 only: the 128-byte id of a new communicator (ncclGetUniqueId)
 *   mdh_comm_init        every rank, collectively: joins (ncclCommInitRank on the renderer's device) and sets
 *                        MDH_OPT_RANK / MDH_OPT_WORLD, which cannot be set by hand while the communicator lives
 *   mdh_comm_destroy     leaves; the renderer is rank 0 of 1 again
 *   mdh_comm_abort       tears the communicator down WITHOUT waiting for collectives in flight
 *                        (ncclCommAbort): what a host's watchdog calls when a peer never arrives
 *   mdh_comm_barrier     mdh_finish + a collective every rank has to reach + host wait
 *   mdh_comm_max_f64     *value = max over the ranks (timing: the slowest rank's wall time)
 *   mdh_comm_reduce_framebuffer
 *                        the ranks' tiles of the last frame summed into `root`'s framebuffer (every pixel is
 *                        non-zero on one rank only, so the sum is the whole frame bit for bit up to the sign of
 *                        zeros): what mdh_read_framebuffer / the window of rank `root` then shows.  Not part of
 *                        a frame; a host that presents the image calls it, a benchmark does not. */
#define MDH_COMM_ID_BYTES 128
int32_t mdh_comm_unique_id(uint8_t id_out[MDH_COMM_ID_BYTES]);
/* MDH_OK when this process can load librccl (what the ranks other than 0 ask before everybody enters mdh_comm_init) */
int32_t mdh_comm_available(void);
int32_t mdh_comm_init(mdh_renderer *r, const uint8_t id[MDH_COMM_ID_BYTES], int32_t rank, int32_t world);
int32_t mdh_comm_destroy(mdh_renderer *r);
int32_t mdh_comm_abort(mdh_renderer *r);
int32_t mdh_comm_barrier(mdh_renderer *r);
int32_t mdh_comm_max_f64(mdh_renderer *r, double *value);
int32_t mdh_comm_reduce_framebuffer(mdh_renderer *r, int32_t root);

/* ---- the same sharded frame WITHOUT a collective library: the peer exchange ("a hand-rolled P2P
 * fan-out").  Every rank exports the interprocess handles (hipIpcGetMemHandle) of its radiance atlases and of a block of
 * frame numbers in device memory; the host hands every rank's 512 bytes to every rank (a file, a pipe, whatever it used
 * for the communicator id); mdh_peer_init opens the peers' handles.  From then on mdh_render is the sharded frame of
 * mdh_comm_init, its exchange step being COPIES ordered on the device: behind its radiance pass a rank stores the
 * frame's number into its block; for each peer it enqueues one wavefront that polls the peer's number until it has
 * reached this frame's, and behind it the copy of the peer's slice out of the peer's atlas into its own
 * (hipMemcpyAsync, device to device) -- all on the probe stream, no host waits, frames stay in flight.  The irradiance
 * pass runs for all probes on every rank (MDH_OPT_IRRADIANCE_ALL must be on).  It is the fall-back between RCCL and the
 * exchange through host memory, and the one device-resident exchange that several processes can run on ONE GPU (RCCL
 * refuses two ranks of a communicator on one device).  The ranks must be processes of one node (one process per rank)
 * and must all render the same frames; a peer that never arrives ends the wait after a few seconds and the next
 * mdh_render / mdh_finish returns MDH_E_COMM.
 *   mdh_peer_export   this rank's handles (MDH_PEER_BLOB_BYTES bytes); starts a new session at frame 0
 *   mdh_peer_init     every rank, with all ranks' blobs in rank order; sets MDH_OPT_RANK / MDH_OPT_WORLD
 *   mdh_comm_destroy / mdh_comm_abort   leave (as for a communicator); mdh_comm_barrier, mdh_comm_max_f64 and
 *                     mdh_comm_reduce_framebuffer need a communicator and return MDH_E_STATE here */
#define MDH_PEER_BLOB_BYTES 512
int32_t mdh_peer_export(mdh_renderer *r, uint8_t blob_out[MDH_PEER_BLOB_BYTES]);
int32_t mdh_peer_init(mdh_renderer *r, const uint8_t *blobs /* world x MDH_PEER_BLOB_BYTES */, int32_t rank, int32_t world);

/* replaces Swap_Buffers (renderers.adb:320): linear RGB floats, H*W*3, row 0 = top.
 * In a sharded run only this rank's tiles are written, the rest is 0. */
int32_t mdh_read_framebuffer(mdh_renderer *r, float *rgb_out);
/* Swap_Buffers itself (renderers.adb:320): what the reference's window shows.  The default framebuffer of
 * that window is RGBA8 without sRGB encoding, so the last frame's colours are clamped to [0, 1] and
 * converted to the nearest of 256 levels per channel (OpenGL 4.3 core 2.3.5.1; ties to even, NaN -> 0,
 * alpha = 255), on the device.  mdh_swap_buffers enqueues that conversion and the copy into a pinned host
 * buffer behind the frame and returns without waiting: frames stay in flight (MDH_OPT_FRAME_OVERLAP)
 * and the copy of one frame runs beside the passes of the next.  mdh_front_buffer waits for the most
 * recent swap only and returns its pixels: H*W*4 bytes, R G B A, row 0 = top, owned by the renderer
 * and valid until the second next mdh_swap_buffers (with MDH_OPT_WINDOW also: until three more
 * screen passes have been started); *swap_count (may be NULL) is the number of swaps so far.
 * With MDH_OPT_WINDOW = 1 the screen pass has stored the pixels in host memory already and the swap
 * only marks them.  In a sharded run only this rank's tiles are written, the rest is 0. */
int32_t mdh_swap_buffers(mdh_renderer *r);
int32_t mdh_front_buffer(mdh_renderer *r, const uint8_t **rgba, int64_t *swap_count);
/* primary-ray geometry buffer (needs MDH_OPT_GBUFFER): per pixel the flat
 * primitive index of closest_primitive_info (-1 = miss), the march length t
 * and the number of SDF evaluations of the primary march */
int32_t mdh_read_gbuffer(mdh_renderer *r, int32_t *index_out, float *t_out, int32_t *steps_out);

/* texture contents as the reference's 2-D images (row 0 = normalised y of 0),
 * `channels` floats per texel (3, or 4 for scattering); out may be NULL to
 * query the size only */
int32_t mdh_read_texture(mdh_renderer *r, int32_t tex, float *out, int32_t *width, int32_t *height,
                         int32_t *channels);
/* deterministic warm start / checkpoint of the DDGI state (same layout) */
int32_t mdh_write_texture(mdh_renderer *r, int32_t tex, const float *in, int32_t width, int32_t height,
                          int32_t channels);

/* probe-major atlas slices through host memory, [probe][res][res][3] floats:
 * the exchange step of a sharded run when the ranks have no device collective */
int32_t mdh_read_atlas_slice(mdh_renderer *r, int32_t tex, int32_t probe_begin, int32_t n_probes, float *out);
int32_t mdh_write_atlas_slice(mdh_renderer *r, int32_t tex, int32_t probe_begin, int32_t n_probes,
                              const float *in);

/* device-resident atlas slices for callers that bring an exchange of their own (mdh_comm_init needs none of this):
 * pointer to the probe-major atlas, its total byte size and the byte range
 * [offset, offset+bytes) this rank owns */
int32_t mdh_atlas_device_ptr(mdh_renderer *r, int32_t tex, void **dptr, int64_t *total_bytes,
                             int64_t *own_offset, int64_t *own_bytes);
/* the HIP stream (hipStream_t) every pass is enqueued on */
int32_t mdh_stream(mdh_renderer *r, void **stream);
/* enqueue on the caller's stream instead (e.g. the one an RCCL communicator is
 * ordered with); NULL returns to the renderer's own stream */
int32_t mdh_set_stream(mdh_renderer *r, void *stream);
/* the stream the probe passes of an open frame run on (hipStream_t) */
int32_t mdh_probe_stream(mdh_renderer *r, void **stream);

/* Renderers.Eval_Distance_To (madarch-renderers.adb:499-526), batched: for
 * each of n points the closest distance over the listed kinds (initial
 * closest 1.0e10) and the normal of the arg-min primitive.  n = 1 is the
 * reference call.  Runs beside the frames in flight (a stream of its own) and
 * returns when its own results are on the host. */
int32_t mdh_eval_distance_to(mdh_renderer *r, int32_t n, const float *points_xyz,
                             const int32_t *kind_ixs, int32_t n_kinds, float *normals_xyz_out,
                             float *dist_out);

/* Ray queries: the shaders' raycast, raycast_visibility and softshadows (glsl/raymarching.glsl:4-56) for n rays of the
 * host's -- what a ray hits, whether two points see each other, how much of a light reaches a point.  All arrays are host
 * memory; origins and directions are 3 n floats, and a direction is used as given (not normalised), as in the shaders.
 * Like mdh_eval_distance_to the calls run on the query stream beside the frames in flight, see pending Set_Primitive /
 * Add_Primitive / Update_Partitioning, and return when their results are on the host.  They go through the space
 * partition (or the triangle BVH) where the scene has one, as every pass does.  They edit nothing: the probe-settle run
 * and the radiance and screen replays go on across them.  n = 0 is MDH_OK.
 *   MDH_E_INVALID  a null renderer or required array, n < 0, a non-finite origin, direction, tmax, tmin or k, a tmax
 *                  above the scene's max_dist, tmin < 0 -- checked on the host before anything is launched
 *   MDH_E_STATE    the scene declares a user-defined primitive or light kind: neither the kernels' interpreter nor the
 *                  hiprtc build of such scenes answers ray queries (built-in kinds only)
 * The shaders' marches have no step cap; here a step that no longer moves the ray (total + dist == total in fp32: a far
 * point along a grazing ray, where the shader would never return) ends the march -- raycast reports a miss, visibility
 * 1, soft shadows the value reached.
 *
 * mdh_raycast: raycast up to the scene's max_dist.  hit 0 / 1; index in the numbering of mdh_read_gbuffer, -1 for a
 * miss; t the distance marched, 0 for a miss; steps the SDF evaluations, on a miss too; pos = org + dir * t as the march
 * computed it; normal = primitive_info's normal of primitive `index` at pos; pos and normal 0 for a miss.  Every output
 * except hit_out may be NULL. */
int32_t mdh_raycast(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, int32_t *hit_out,
                    int32_t *index_out, float *t_out, int32_t *steps_out, float *pos_xyz_out, float *normal_xyz_out);
/* raycast_visibility: 1.0 when ray i reaches tmax[i] (<= max_dist) without a hit, 0.0 otherwise */
int32_t mdh_raycast_visibility(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, const float *tmax,
                               float *vis_out);
/* softshadows with the shader's min_dist (tmin >= 0), max_dist (tmax[i] <= max_dist) and k: 0 behind an occluder, else
 * the smallest k * d / max (0, t - y) along the ray, at most 1 */
int32_t mdh_softshadows(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, float tmin, const float *tmax,
                        float k, float *out);
/* under MDH_OPT_TIMING: the time of the last ray query's kernel in milliseconds, between two events on the query stream
 * (without the copies to and from the device); 0 before the first timed query */
int32_t mdh_ray_query_time(mdh_renderer *r, double *kernel_ms);

/* The same three queries for rays that live on the device: every array is memory the renderer's device can address
 * (its own memory, page-locked host memory, managed memory), with the meaning, the layout and the optional outputs of
 * the calls above.  `stream` is a hipStream_t (NULL: the default stream, which is PyTorch's).  The calls are asynchronous
 * and ordered with that stream: the kernel starts after everything enqueued on `stream` before the call, whatever is
 * enqueued on `stream` after the call sees the answers, and the call returns without waiting for the device.  The arrays
 * stay the caller's and must live until the query has ended.  The scene is the one committed at the call, pending edits
 * included; the calls edit nothing, as above.  n = 0 is MDH_OK without a launch.
 *   MDH_E_INVALID  a null renderer or required array, n < 0, tmin < 0, a non-finite tmin or k, and an array that is not
 *                  memory the device addresses (hipPointerGetAttributes: pageable host memory, another device's) or
 *                  that ends outside its allocation -- checked before anything is launched; HIP's error state is cleared
 *   MDH_E_STATE    a scene with a user-defined kind
 * The host cannot look at the rays, so the device does: a ray with a non-finite component, or with a tmax that is not
 * finite or exceeds the scene's max_dist -- what the calls above refuse the whole batch for -- is not marched.
 * mdh_raycast_device answers it with hit = -1, index = -1, t = 0, steps = 0, pos = normal = 0; the other two with the
 * quiet NaN 0x7fc00000.  Every other ray has the bits the calls above give it, whatever MDH_OPT_RAY_STREAM_REFILL and
 * MDH_OPT_RAY_STREAM_GROUPS say: lanes take the next ray from a counter when their own has ended (k_ray_stream). */
int32_t mdh_raycast_device(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, int32_t *hit_out,
                           int32_t *index_out, float *t_out, int32_t *steps_out, float *pos_xyz_out, float *normal_xyz_out,
                           void *stream);
int32_t mdh_raycast_visibility_device(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz,
                                      const float *tmax, float *vis_out, void *stream);
int32_t mdh_softshadows_device(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, float tmin,
                               const float *tmax, float k, float *out, void *stream);
/* blocks until every device query enqueued so far has ended (for callers that read the answers from the host; work on
 * the query's own stream needs no wait).  Under MDH_OPT_TIMING mdh_ray_query_time then reads the last one's kernel; called
 * by itself it waits for that query's end event first. */
int32_t mdh_ray_query_wait(mdh_renderer *r);

/* What a ray sees: pixel_color_probes (glsl/render_probes.glsl:246-291) -- direct light with soft shadows, the DDGI
 * irradiance of the cage, the reflection's radiance tap, ambient occlusion -- along n rays of the host's, through the pixel
 * program the screen pass runs.  Origins and directions are 3 n floats, directions used as given.
 *   mode 0      the reference's fixed mode: pixel_color_probes with the renderer's current MDH_OPT_AO_STEPS and
 *               MDH_OPT_INDIRECT_SPECULAR and with direct specular on, as renderers.adb:136-143 sets the screen shader
 *   mode 2      this library's mode-2 screen pass: direct light times occlusion, no probes
 *   tone_map 0  the linear colour pixel_color_probes returns; a miss is the sky of render_probes.glsl:287 along the ray
 *   tone_map 1  draw_screen.glsl:29 applied to it: the bits the framebuffer would hold
 * rgb_out (3 n floats) is required; hit_out (0 / 1), index_out, t_out and steps_out may be NULL and carry the meaning and
 * the numbering of mdh_read_gbuffer.
 * NO VOLUMETRICS: the fog of glsl/volumetrics.glsl:34-54 is looked up by the fragment's screen position, which a free ray
 * does not have -- the query never composes fog, whatever the renderer's volumetric settings.  (The fog along a free ray
 * is a call of its own: mdh_inscatter_rays below, which a host composes with this call's linear colour.)
 * The call reads the scene committed at the call, pending edits included, and the atlas set a
 * mdh_render_pass (MDH_PASS_SCREEN) issued at the same moment would read: it runs behind the passes that write that set, and
 * no later frame rewrites the set before the query's kernel has ended.  It edits nothing: the probe-settle run and the
 * radiance and screen replays go on across it.  n = 0 is MDH_OK without a launch.
 *   MDH_E_INVALID  a null renderer or required array, n < 0, a mode other than 0 or 2 (mode 1, the normal, is
 *                  mdh_raycast's), and -- mdh_shade_rays, on the host, the whole batch -- a ray that is not shaded (below)
 *   MDH_E_STATE    a scene with a user-defined kind; an open frame; MDH_OPT_INDIRECT_SPECULAR 1 or 3, or 2 over a mip
 *                  chain in use (the screen pass's other variant: not built for rays); a scene outside the bound below
 * The marches of the pixel program have no step cap and no stall guard, so termination is kept by a bound: a ray is
 * shaded only if every component is finite, every origin component is at most 1024 and every direction component at most
 * 2 in magnitude, and the call is refused when the scene's max_dist exceeds 1024 or a light's position or the probe
 * grid's far corner has a component beyond 1024 in magnitude.  Every march parameter then stays below 2^14, where a step
 * of at least epsilon still advances it ("Shading a host's rays"). */
int32_t mdh_shade_rays(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, int32_t mode, int32_t tone_map,
                       float *rgb_out, int32_t *hit_out, int32_t *index_out, float *t_out, int32_t *steps_out);
/* The same call for arrays the device addresses, under the contract of mdh_raycast_device: asynchronous and ordered with
 * `stream` (a hipStream_t; NULL: the default stream), mdh_ray_query_wait is the host's wait, and where every array lives
 * and ends is checked with hipPointerGetAttributes before anything is launched (MDH_E_INVALID).  The host cannot look at
 * the rays, so the lane that takes a ray which is not shaded answers it without marching: the quiet NaN 0x7fc00000 in all
 * three colours, hit = -1, index = -1, t = 0, steps = 0.  Every other ray has the bits mdh_shade_rays gives it. */
int32_t mdh_shade_rays_device(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, int32_t mode,
                              int32_t tone_map, float *rgb_out, int32_t *hit_out, int32_t *index_out, float *t_out,
                              int32_t *steps_out, void *stream);
/* The rays of a width x height frame of the renderer's current camera (glsl/draw_screen.glsl:20-24), 3 width height floats
 * each, rows top first like the framebuffer.  They are computed on the device by the screen pass's own functions and are
 * the frame's rays to the bit: a host jitters, warps or subsamples them and hands them to the calls above.  The device
 * variant is enqueued on `stream` itself.  MDH_E_INVALID: a null renderer or array, a width or height below 1, more than
 * 2^28 pixels, an array the device cannot address. */
int32_t mdh_camera_rays(mdh_renderer *r, int32_t width, int32_t height, float *org_xyz_out, float *dir_xyz_out);
int32_t mdh_camera_rays_device(mdh_renderer *r, int32_t width, int32_t height, float *org_xyz_out, float *dir_xyz_out,
                               void *stream);

/* What light arrives at a point the host owns: the lighting of pixel_color_probes (glsl/render_probes.glsl:253-285) from the
 * hit on, for n points that need not lie on any primitive of the scene -- a host's own rasterised meshes, particles, a light
 * meter, a lightmap baker.  pos_xyz and normal_xyz (3 n floats each) are the shaded point and its normal, used as given
 * (not normalised) as the shaders use them; view_dir_xyz (3 n floats) is the shader's `dir`, the direction the point is seen
 * ALONG, from the eye to the point; material_ids (n) are ids of the renderer's material table, 0-based as mdh_add_material
 * returns them (a host registers its own materials with the calls it has).
 *   mode 0      (compute_direct_lighting + compute_indirect_lighting (sample_irradiance, specular_col)) * ambient occlusion,
 *               with the renderer's MDH_OPT_AO_STEPS and MDH_OPT_INDIRECT_SPECULAR (0 or 2; for 2 the reflection's radiance
 *               tap, sample_radiance_no_specular, from pos, normal and reflect (view_dir, normal)) and direct specular on
 *   mode 2      direct light times occlusion, no probes
 *   mode 3      MDH_POINT_IRRADIANCE: rgb_out = sample_irradiance (pos, normal) (render_probes.glsl:6-69) and nothing else;
 *               view_dir_xyz and material_ids may be NULL and are not read; tone_map must be 0
 *   tone_map 1  (modes 0 and 2) draw_screen.glsl:29 applied, as mdh_shade_rays does
 * NO VOLUMETRICS: never any fog.  A point mdh_raycast found -- its position and normal, the ray's direction, the material
 * mdh_primitive_material names -- gets the bits mdh_shade_rays gives that ray and the frame gives that pixel.
 * The contract is mdh_shade_rays': the call runs on the query stream beside the frames in flight, reads the scene committed
 * at the call, pending edits included, and the atlas set a mdh_render_pass (MDH_PASS_SCREEN) issued at that moment would
 * read, and edits nothing: the probe-settle run and both replays go on across it.  It marches through the space partition
 * or the triangle BVH where the scene has one.  n = 0 is MDH_OK without a launch.
 *   MDH_E_INVALID  a null renderer or required array, n < 0, a mode other than 0, 2 or 3, a tone map in mode 3, and --
 *                  mdh_shade_points, on the host, the whole batch -- a point that is not shaded (below)
 *   MDH_E_STATE    a scene with a user-defined kind; an open frame; in modes 0 and 2 MDH_OPT_INDIRECT_SPECULAR 1 or 3, or 2
 *                  over a mip chain in use; a scene outside the bound of mdh_shade_rays (max_dist, lights, probe grid)
 * The marches have no step cap and no stall guard, so a point is shaded only inside a bound: every component finite, every
 * position component at most 1024 in magnitude, every normal and view-direction component at most 1, the material id
 * inside the table (0 .. 19).  The bound on normals and view directions is TIGHTER than the 2 of a shaded ray's direction:
 * the reflected direction view - 2 dot (normal, view) normal is as long as |view| (1 + 2 |normal|^2), 7 sqrt 3 for
 * components of 1 and 50 sqrt 3 for components of 2, and only the former keeps the reflection's hit -- and the shadow and
 * visibility rays that start there -- below 2^14 ("Lighting a host's points"). */
#define MDH_POINT_IRRADIANCE 3
int32_t mdh_shade_points(mdh_renderer *r, int32_t n, const float *pos_xyz, const float *normal_xyz, const float *view_dir_xyz,
                         const int32_t *material_ids, int32_t mode, int32_t tone_map, float *rgb_out);
/* The same call for arrays the device addresses, under the contract of mdh_shade_rays_device: asynchronous and ordered with
 * `stream` (a hipStream_t; NULL: the default stream), mdh_ray_query_wait is the host's wait and mdh_ray_query_time times
 * the kernel, and where every array lives and ends is checked with hipPointerGetAttributes before anything is launched
 * (MDH_E_INVALID).  The host cannot look at the points, so the lane that takes a point which is not shaded answers it
 * without marching: the quiet NaN 0x7fc00000 in all three colours.  Every other point has the bits mdh_shade_points gives. */
int32_t mdh_shade_points_device(mdh_renderer *r, int32_t n, const float *pos_xyz, const float *normal_xyz,
                                const float *view_dir_xyz, const int32_t *material_ids, int32_t mode, int32_t tone_map,
                                float *rgb_out, void *stream);
/* The material id of primitive index[q] -- the numbering of mdh_read_gbuffer and mdh_raycast -- in the scene as it stands,
 * pending edits included: a lookup on the host, no launch.  -1 for -1 and for an index no primitive has.  It feeds
 * mdh_raycast's hits to mdh_shade_points.  MDH_E_STATE: a scene with a user-defined kind (its material is a program). */
int32_t mdh_primitive_material(mdh_renderer *r, int32_t n, const int32_t *index, int32_t *material_out);

/* Ground truth for the probes: a path tracer along n rays of the host's.  For every ray and sample: mask = 1, rgb = 0, then up
 * to bounces + 1 segments, each the shaders' raycast to max_dist.  A miss adds mask * sky (the expression of
 * glsl/render_probes.glsl:287 along the segment) and ends the path.  A hit adds mask * compute_direct_lighting
 * (glsl/lighting.glsl:1-40, direct specular on), multiplies the mask by the hit's albedo and goes on from
 * P + normal * 0.05 * 5 along the sampler's direction (mdh_path_scatter below).  It restates the reference's
 * glsl/render_path.glsl, which the reference never includes, with three deviations: the sky is masked, it is added once, and
 * the next origin is offset from the surface.  Ray i has id id_first + i; the random numbers of a path depend on (seed, id,
 * sample, bounce) and on nothing else -- not on the batch or its order.
 * rgb_accum (3 n floats, linear, IN AND OUT) holds sums: the call adds samples sample_first .. sample_first + sample_count - 1
 * to what the array holds, in that order, so a run of samples split over several calls has the bits of one call; the host
 * divides by the count.  hit_out (0 / 1), index_out and t_out may be NULL and describe the primary segment, as mdh_shade_rays'.
 * NO VOLUMETRICS: the query never composes fog (mdh_inscatter_rays below gathers it along a ray).  It reads no atlas, and MDH_OPT_AO_STEPS and MDH_OPT_INDIRECT_SPECULAR do
 * not enter it.  Otherwise the contract is mdh_shade_rays': the call runs on the query stream behind the same fences, reads
 * the scene committed at the call, pending edits included, and edits nothing: the probe-settle run and both replays go on
 * across it.  n = 0 or sample_count = 0 is MDH_OK without a launch.  Every refusal happens before a launch:
 *   MDH_E_INVALID  a null renderer or required array, n < 0, sample_first < 0, sample_count < 0, a sum of the two beyond
 *                  2^31 - 1, bounces outside 0 .. 6, and -- mdh_path_trace, on the host, the whole batch -- a ray outside
 *                  the bound of mdh_shade_rays (finite, origin within 1024, direction within 2 per component) or with a
 *                  direction of zero
 *   MDH_E_STATE    a scene with a user-defined kind; an open frame; a max_dist above 1024 or a light beyond 1024
 * The marches have no stall guard.  Behind the first segment every direction is a unit vector, so a bounce moves the shaded
 * point by less than max_dist + 0.25: six bounces keep every march parameter below 13 246 < 2^14 (DESIGN.md section 4,
 * "Path tracing a host's rays"). */
int32_t mdh_path_trace(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, uint32_t seed, uint32_t id_first,
                       int32_t sample_first, int32_t sample_count, int32_t bounces, float *rgb_accum, int32_t *hit_out,
                       int32_t *index_out, float *t_out);
/* The same call for arrays the device addresses, under the contract of mdh_shade_rays_device: asynchronous and ordered with
 * `stream`, mdh_ray_query_wait is the host's wait and mdh_ray_query_time times the kernel, and where every array lives and
 * ends is checked with hipPointerGetAttributes before anything is launched (MDH_E_INVALID).  The lane that takes a ray
 * outside the bound, or with a zero direction, answers it without marching: the quiet NaN 0x7fc00000 in all three colours, hit = -1, index = -1, t = 0.
 * Every other ray has the bits mdh_path_trace gives it.  The sums stay on the device from call to call. */
int32_t mdh_path_trace_device(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, uint32_t seed,
                              uint32_t id_first, int32_t sample_first, int32_t sample_count, int32_t bounces, float *rgb_accum,
                              int32_t *hit_out, int32_t *index_out, float *t_out, void *stream);
/* The sampler by itself, on the host: no launch and no renderer.  dir_out[i] is the direction the path of ray id_first + i
 * takes behind bounce `bounce` of sample `sample`, having arrived along dir_xyz[i] at a surface with normal normal_xyz[i]
 * (any length but 0) and roughness[i]: cosine-weighted about the normal with probability `roughness`, else the mirror
 * direction widened by the roughness; always normalised.  The functions are the ones the lanes of mdh_path_trace call
 * (csrc/mdh_path.h): the same bits, so a host can continue paths its own way or compose the whole estimator from mdh_raycast,
 * mdh_primitive_material and mdh_shade_points.  A component that is not finite (a zero normal, a mirror direction that
 * cancels) ends the path in mdh_path_trace.  MDH_E_INVALID: n, sample or bounce below 0, a null array with n > 0. */
int32_t mdh_path_scatter(int32_t n, const float *dir_xyz, const float *normal_xyz, const float *roughness, uint32_t seed,
                         uint32_t id_first, int32_t sample, int32_t bounce, float *dir_out);

/* A PATH-TRACED FRAME: mdh_path_trace's estimator over the pixels of a frame of the camera, with the sums kept on the device
 * from call to call -- no rays fetched, nothing carried in and out per slice of samples --, sub-pixel jitter, and the resolve
 * on the device.  Pixel (i, j) of the width x height frame, row 0 at the top, has the ray id j * width + i: the numbering of
 * mdh_camera_rays with id_first = 0.  For sample s its ray is camera_ray (u, v) (glsl/draw_screen.glsl:20-24) at
 *     jx = jitter ? path_u01 (seed, id, s, 0, 3) : 0.5        jy = jitter ? path_u01 (seed, id, s, 0, 4) : 0.5
 *     u = ((float)(2 i) + 2 jx) / (float) width - 1           v = -(((float)(2 j) + 2 jy) / (float) height - 1)
 * every step one binary32 operation (path_u01: csrc/mdh_path.h; the sampler takes dimensions 0 .. 2 of every bounce, so 3 and 4
 * of bounce 0 are taken by nobody).  A jittered ray stays inside its pixel's footprint; without jitter the numerator is
 * (float)(2 i + 1) and the rays are mdh_camera_rays' to the bit.  NO VOLUMETRICS, as in mdh_path_trace.
 *
 * mdh_path_frame_begin opens, or restarts from zero, the renderer's accumulator of width x height pixels -- three fp32 sums a
 * pixel in device memory; the size is free, not the window's, at most MDH_PATH_FRAME_MAX_PIXELS pixels -- and fixes seed,
 * bounces (0 .. 6) and jitter (0 / 1).  It CAPTURES THE CAMERA as it stands: later mdh_set_camera_position /
 * mdh_set_camera_orientation do not smear a running accumulation.
 *
 * mdh_path_frame_accumulate adds samples S .. S + sample_count - 1 to every pixel, S being the samples accumulated so far, each
 * pixel's in sample order: a run of samples split over several calls has the bits of one call, and without jitter the sums
 * are those of mdh_path_trace over mdh_camera_rays' rays with sample_first = S.  It runs on the query stream under
 * mdh_path_trace's contract -- the scene committed at the call, pending edits included; nothing edited: the probe-settle run
 * and both replays go on -- and RETURNS WITHOUT WAITING for the device: there is nothing to copy.  mdh_ray_query_time times its
 * kernel under MDH_OPT_TIMING (after mdh_ray_query_wait, or by itself).  The accumulator does not notice an edit of the scene:
 * RESTARTING AFTER AN EDIT IS THE HOST'S BUSINESS (mdh_path_frame_begin again).  sample_count = 0 is MDH_OK without a launch.
 * A pixel whose ray is outside mdh_path_trace's bound (a camera moved beyond 1024) is not marched: its three sums become the
 * quiet NaN 0x7fc00000 and stay so.
 *
 * mdh_path_frame_read is the resolve, on the device; every output may be NULL.  rgb_out (3 floats a pixel) = sum / (float) S,
 * one binary32 division a channel, and with tone_map = 1 glsl/draw_screen.glsl:29 applied to it as mdh_shade_rays applies it;
 * rgba8_out (one uint32 a pixel, R in the low byte) = that colour with alpha 1 as the window's RGBA8 pixels hold a framebuffer
 * pixel (MDH_OPT_WINDOW; a NaN shows as 0); sums_out (3 floats a pixel) = the raw sums; samples_out = S.  Rows are top first,
 * as in the framebuffer.  The host form waits and copies.  mdh_path_frame_read_device writes arrays the device addresses
 * (samples_out stays the host's) under the contract of mdh_raycast_device: checked with hipPointerGetAttributes before anything
 * is launched, asynchronous and ordered with `stream`, mdh_ray_query_wait is the host's wait.
 *
 * mdh_path_frame_rays gives the rays the accumulator gives its pixels for sample `sample` (3 width height floats each), computed
 * on the device by the functions the accumulating kernel calls: a host inspects or bends them, or chains the public queries
 * over them.  The device form is enqueued on `stream` itself, as mdh_camera_rays_device.
 *
 * mdh_path_frame_info reports the accumulator's state (any pointer may be NULL; all zeros while none is open);
 * mdh_path_frame_end frees it, and so does mdh_destroy.
 *
 * The accumulator ignores MDH_OPT_RANK / MDH_OPT_WORLD, as every query does.  Every refusal happens before any launch or
 * allocation:
 *   MDH_E_INVALID  a null renderer; a width or height below 1 or more than MDH_PATH_FRAME_MAX_PIXELS pixels; bounces outside
 *                  0 .. 6; a jitter or tone_map other than 0 / 1; a negative sample_count or sample; the samples so far and
 *                  sample_count beyond 2^31 - 1; a null array of mdh_path_frame_rays; an array the device cannot address
 *   MDH_E_STATE    no accumulator open (accumulate, read, rays); no sample accumulated yet (read: there is no 0 / 0 image);
 *                  and, for begin and accumulate, what mdh_path_trace refuses: a scene with a user-defined kind, an open
 *                  frame, a max_dist above 1024 or a light beyond 1024 */
#define MDH_PATH_FRAME_MAX_PIXELS 67108864 /* 2^26: 805 MB of sums, room above a 4096 x 4096 frame */
int32_t mdh_path_frame_begin(mdh_renderer *r, int32_t width, int32_t height, uint32_t seed, int32_t bounces, int32_t jitter);
int32_t mdh_path_frame_accumulate(mdh_renderer *r, int32_t sample_count);
int32_t mdh_path_frame_read(mdh_renderer *r, int32_t tone_map, float *rgb_out, uint32_t *rgba8_out, float *sums_out,
                            int32_t *samples_out);
int32_t mdh_path_frame_read_device(mdh_renderer *r, int32_t tone_map, float *rgb_out, uint32_t *rgba8_out, float *sums_out,
                                   int32_t *samples_out, void *stream);
int32_t mdh_path_frame_rays(mdh_renderer *r, int32_t sample, float *org_xyz_out, float *dir_xyz_out);
int32_t mdh_path_frame_rays_device(mdh_renderer *r, int32_t sample, float *org_xyz_out, float *dir_xyz_out, void *stream);
int32_t mdh_path_frame_info(mdh_renderer *r, int32_t *width, int32_t *height, int32_t *samples, int32_t *bounces,
                            int32_t *jitter);
int32_t mdh_path_frame_end(mdh_renderer *r);
/* The jitter by itself, on the host: no launch and no renderer, the inline functions the lanes call (csrc/mdh_path.h), the
 * same bits.  uv_out[2 q], uv_out[2 q + 1] = (u, v) above of the pixel with id id_first + q of a width x height frame for
 * sample `sample`.  MDH_E_INVALID: a size as mdh_path_frame_begin refuses it, n or sample below 0, a jitter other than 0 / 1,
 * ids beyond the frame's pixels, a null array with n > 0. */
int32_t mdh_path_pixel_uv(int32_t width, int32_t height, uint32_t seed, uint32_t id_first, int32_t n, int32_t sample,
                          int32_t jitter, float *uv_out);

/* AN ADAPTIVE PATH-TRACED FRAME: the accumulator above with a per-pixel variance estimate, a stopping rule and a deterministic
 * compaction of the pixels still running.  Beside its three sums a pixel holds an int32 count n of its completed samples and
 * two fp32 moments m1, m2.  When a sample of a pixel completes with radiance (r, g, b), every step one binary32 operation,
 * unfused:
 *     y = (r + g) + b      acc = acc + rgb      m1 = m1 + y      m2 = m2 + y * y  (the product rounded, then the sum)      n = n + 1
 * A pixel's k-th sample has SAMPLE INDEX k, its own count and not a global one: pixel id with count n holds exactly samples
 * 0 .. n - 1 of (seed, id), and its sums are mdh_path_trace's over those samples.  The rule (csrc/mdh_path.h: path_pixel_active,
 * the one inline function the lanes and mdh_path_pixel_active call):
 *     if (n >= max_samples) return false;
 *     if (m1 or m2 is a NaN) return false;          a pixel that was not traced does not count up: it retires here
 *     if (n <  min_samples) return true;
 *     c = (float) n;  mean = m1 / c;  q = m2 / c;
 *     var = q - mean * mean;                        the product rounded, then the difference
 *     e   = var / c;                                the variance of the mean
 *     lim = tolerance * (mean + floor);
 *     return e > lim * lim;                         any NaN: false -- the pixel retires
 * A var that rounds negative retires the pixel; tolerance = 0 keeps every pixel with e > 0 running to max_samples and retires
 * pixels of exactly zero variance at min_samples.  THIS IS A STOPPING RULE ON A BIASED VARIANCE ESTIMATE: the resolved image is
 * not claimed to be unbiased, and min_samples is the host's guard.
 *
 * mdh_path_frame_begin_adaptive is mdh_path_frame_begin plus the four parameters -- the same checks, the same captured camera, the
 * same query stream -- with 1 <= min_samples <= max_samples <= 2^24 and tolerance, floor finite and >= 0.  It opens, or
 * restarts, the renderer's one accumulator as an adaptive one; mdh_path_frame_begin still opens a plain one.
 *
 * On an adaptive frame mdh_path_frame_accumulate is ONE ROUND: every pixel active under the rule at the round's start takes
 * min (sample_count, max_samples - n) more samples, and nothing else is touched.  THE RULE IS EVALUATED AT ROUND BOUNDARIES
 * ONLY: TWO ROUNDS OF 2 ARE NOT ONE ROUND OF 4.  It returns without waiting, and no host read-back happens between or inside
 * rounds: the host never learns the active count unless it asks (mdh_path_frame_stats).  A pixel whose ray is outside
 * mdh_path_trace's bound is not marched: its sums, m1 and m2 become the quiet NaN 0x7fc00000, n does not advance, and the rule
 * retires it.  mdh_path_frame_info's samples is the largest count a pixel can hold: the rounds' sum clamped to max_samples.
 * mdh_path_frame_read / _read_device give rgb = sum / (float) n of the pixel; sums_out is the raw sums, samples_out as _info.
 *
 * mdh_path_frame_stats: count_out = n (width height int32), moments_out = (m1, m2) a pixel (2 width height floats), *active = the
 * pixels active under the rule now, *total_samples = the sum of n.  Any pointer may be NULL.  The host form waits and copies;
 * mdh_path_frame_stats_device writes arrays the device addresses, checked before anything is launched and ordered with `stream`
 * as mdh_path_frame_read_device -- there active and total_samples are two int64 words in device memory, aligned to 8 bytes.
 * The two scalars cost a serial pass of one workgroup over all pixels (W H / 256 pixels a thread): a diagnostic, not
 * something to ask behind every round of a large frame.
 *
 * MEMORY.  Beside the 12 bytes of sums a pixel an adaptive frame holds 12 bytes a pixel (n, m1, m2) and, for the list of running
 * pixels, 256 bytes per 8 x 8 TILE (64 slots of 4 bytes, cut tiles included) plus 4 bytes per 256 slots: 28 bytes a pixel for a
 * frame of whole tiles, but a frame one pixel wide pays 256 bytes for every 8 pixels -- 1 x 2^26 asks for 2 GiB of list.
 *
 * mdh_path_pixel_active is the rule by itself on the host, no renderer and no device: active_out[q] = 0 / 1 for the state
 * (count[q], m1[q], m2[q]).
 *
 * Every refusal happens before any launch or allocation:
 *   MDH_E_INVALID  what mdh_path_frame_begin refuses; min_samples below 1 or above max_samples, max_samples above 2^24, a
 *                  tolerance or floor that is negative or not finite; a negative n_pixels or a null array with n_pixels > 0
 *                  (mdh_path_pixel_active); an array the device cannot address, a 64-bit word that is not aligned (_stats_device)
 *   MDH_E_STATE    mdh_path_frame_stats on a plain frame or with none open; for begin, what mdh_path_frame_begin refuses */
int32_t mdh_path_frame_begin_adaptive(mdh_renderer *r, int32_t width, int32_t height, uint32_t seed, int32_t bounces, int32_t jitter,
                                      int32_t min_samples, int32_t max_samples, float tolerance, float floor);
int32_t mdh_path_frame_stats(mdh_renderer *r, int32_t *count_out, float *moments_out, int64_t *active, int64_t *total_samples);
int32_t mdh_path_frame_stats_device(mdh_renderer *r, int32_t *count_out, float *moments_out, int64_t *active,
                                    int64_t *total_samples, void *stream);
int32_t mdh_path_pixel_active(int32_t n_pixels, const int32_t *count, const float *m1, const float *m2, int32_t min_samples,
                              int32_t max_samples, float tolerance, float floor, uint8_t *active_out);

/* The lights' fog for points and rays of the host's: the participating medium of glsl/volumetrics.glsl without the froxel
 * grid, the screen-space scattering texture or the pinhole camera they are bound to.  All arrays are host memory; positions,
 * origins and directions are 3 n floats and a direction is used as given (not normalised), as in the shaders.
 *
 * mdh_inscatter_points: rgb_out[i] = sample_lights (pos_i, dir_i) of glsl/compute_frustrum_visibility.glsl:8-19 -- over all
 * lights in the light loop's order, result += ((radiance * (exp (-L_dist tau) * visibility)) * tau) *
 * henvey_greenstein_phase (L, dir), with sample_light's normal (1, 0, 0) and tau = 0.1: operation for operation what the
 * visibility pass stores for a froxel, so a froxel's own sample point and direction give the froxel texture's bits.  With f
 * given (n floats; may be NULL) the result is multiplied by exp (-f_i tau), one multiplication per channel: the product
 * the scattering pass forms per step, with the library's exp, so that a host can rebuild a ray's sum.
 *
 * mdh_inscatter_rays: the serial loop of glsl/accumulate_scattering.glsl:17-28 with the integrand evaluated, not tapped:
 *     len_i = march ? min (length (to - org), tmax_i) : tmax_i
 *             (to = org + dir * tmax_i; the shaders' raycast to the scene's max_dist, on a hit to = org + dir * t)
 *     L = 0;  for (f = 0; f < len_i; f += step)  L = L + inscatter ((dir * f) + org, dir) * exp (-f tau)
 *     rgb_out[i] = L * step;  len_out[i] = len_i;  steps_out[i] = the loop's turns
 * in fp32 and in this order: f runs through the values of repeated addition, not through k * step, and the sample point is
 * formed as (dir * f) + org per component.  len_out and steps_out may be NULL.  The answer does not depend on the froxel or
 * scattering settings and needs no volumetrics in the renderer.  A scene without lights answers zeros.
 *
 * The contract is the ray queries' (mdh_raycast above): the calls run on the query stream beside the frames in flight, see
 * pending edits, go through the space partition or the triangle BVH where the scene has one, read no atlas and edit
 * nothing: the probe-settle run and both replays go on across them.  mdh_ray_query_time times their kernel under
 * MDH_OPT_TIMING.  The visibility rays and the length's march carry the ray queries' stall guard; a ray's work is bounded by
 * tmax <= max_dist and max_dist / step <= MDH_INSCATTER_MAX_STEPS.  n = 0 is MDH_OK without a launch.  Every refusal
 * happens before anything is launched:
 *   MDH_E_INVALID  a null renderer or required array, n < 0, march other than 0 or 1, a step that is not finite or not
 *                  above 0, max_dist / step above MDH_INSCATTER_MAX_STEPS; a non-finite position, origin, direction or
 *                  f; a tmax that is not finite, is negative or exceeds the scene's max_dist
 *   MDH_E_STATE    a scene with a user-defined kind */
#define MDH_INSCATTER_MAX_STEPS 4096
int32_t mdh_inscatter_points(mdh_renderer *r, int32_t n, const float *pos_xyz, const float *dir_xyz, const float *f,
                             float *rgb_out);
int32_t mdh_inscatter_rays(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, const float *tmax,
                           int32_t march, float step, float *rgb_out, float *len_out, int32_t *steps_out);
/* The same calls for arrays the device addresses, under the contract of mdh_raycast_device: asynchronous and ordered with
 * `stream` (a hipStream_t; NULL: the default stream), mdh_ray_query_wait is the host's wait, and where every array lives
 * and ends is checked with hipPointerGetAttributes before anything is launched (MDH_E_INVALID; HIP's error state is
 * cleared).  The host cannot look at the values, so the device does: a point or ray the calls above would refuse the batch
 * for is not marched -- its rgb and len are the quiet NaN 0x7fc00000 and its steps -1.  Every other one has the bits the
 * calls above give it. */
int32_t mdh_inscatter_points_device(mdh_renderer *r, int32_t n, const float *pos_xyz, const float *dir_xyz, const float *f,
                                    float *rgb_out, void *stream);
int32_t mdh_inscatter_rays_device(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, const float *tmax,
                                  int32_t march, float step, float *rgb_out, float *len_out, int32_t *steps_out,
                                  void *stream);

/* SWEPT SPHERES AND CONTACTS, for a host that owns moving bodies (the reference's examples/ball_game asks
 * Eval_Distance_To for each ball's new centre: a point test, which a long step carries through a thin obstacle).
 *
 * mdh_spherecast sweeps a sphere of radius radius[i] (NULL: 0) with its centre along ray i up to tmax[i] (NULL: the scene's
 * max_dist) and reports the first contact.  The march is raycast's (glsl/raymarching.glsl:25-37) with the distance
 * fl (D (org + dir * total) - radius) and the bound tmax:
 *    for (total = 0; total < tmax;) { dist = D (p) - radius; ++steps; if (dist < epsilon) hit at t = total;
 *                                     [total + dist == total: a miss]  total += dist }
 * so radius = 0 up to max_dist over the whole scene is mdh_raycast bit for bit, and a sphere that overlaps something at
 * its origin hits at t = 0 with one step.  pos is the CENTRE at contact, org + dir * t as the march computed it; normal is
 * the normal of primitive `index` at that centre, as Eval_Distance_To gives it at a ball's centre (the touching point is
 * pos - normal * radius).  On a miss index = -1 and t, pos and normal are 0.  All outputs but hit_out may be NULL.
 *
 * mdh_contacts evaluates once at each centre: dist = fl (D (centre) - radius), negative where the sphere penetrates, index
 * the closest primitive and normal its normal at the centre; where no instance exists dist = 1.0e10 - radius, index = -1
 * and normal = 0.  index_out and normal_out may be NULL.
 *
 * D: n_kinds = 0 -- the scene as every pass and mdh_raycast see it, through the space partition (its borders and Index_Count
 * included) or the triangle BVH where the scene has one.  n_kinds > 0 -- the exact minimum over the committed instances of
 * the listed kinds in the order listed, as mdh_eval_distance_to scans them (the lowest index wins a tie, no partition is
 * consulted), always with the shaders' division: MDH_OPT_ADA_EVAL_DIV is ignored, a march needs a distance.  A ball that
 * is itself a sphere of the scene lists the kinds it collides with, as the reference's query does.  index is in
 * mdh_read_gbuffer's numbering either way.
 *
 * The contract is the ray queries' (mdh_raycast above): the query stream beside the frames in flight, pending edits seen,
 * nothing edited -- the probe-settle run and both replays go on across the calls, unlike across mdh_eval_distance_to --,
 * the stall guard in the march, mdh_ray_query_time under MDH_OPT_TIMING.  n = 0 is MDH_OK without a launch.  Every refusal
 * happens before anything is launched:
 *   MDH_E_INVALID  a null renderer or required array, n < 0, n_kinds outside 0 .. MDH_MAX_KINDS or a kind index outside the
 *                  scene's kinds; a non-finite origin, direction, centre, radius or tmax; a radius or a tmax below 0 or above
 *                  the scene's max_dist
 *   MDH_E_STATE    a scene with a user-defined kind */
int32_t mdh_spherecast(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, const float *radius,
                       const float *tmax, const int32_t *kind_ixs, int32_t n_kinds, int32_t *hit_out, int32_t *index_out,
                       float *t_out, int32_t *steps_out, float *pos_xyz_out, float *normal_xyz_out);
int32_t mdh_contacts(mdh_renderer *r, int32_t n, const float *centre_xyz, const float *radius, const int32_t *kind_ixs,
                     int32_t n_kinds, float *dist_out, int32_t *index_out, float *normal_xyz_out);
/* The same calls for arrays the device addresses (kind_ixs stays the host's), under the contract of mdh_raycast_device:
 * asynchronous and ordered with `stream`, mdh_ray_query_wait is the host's wait, where every array lives and ends is checked
 * before anything is launched, and MDH_OPT_RAY_STREAM_REFILL / _GROUPS shape the whole-scene sweep's launch.  A ray the calls
 * above would refuse the batch for is answered without a march as mdh_raycast_device answers it (hit = -1, index = -1, the
 * rest 0); such a centre with dist = the quiet NaN 0x7fc00000, index = -1 and normal = 0. */
int32_t mdh_spherecast_device(mdh_renderer *r, int32_t n, const float *org_xyz, const float *dir_xyz, const float *radius,
                              const float *tmax, const int32_t *kind_ixs, int32_t n_kinds, int32_t *hit_out,
                              int32_t *index_out, float *t_out, int32_t *steps_out, float *pos_xyz_out,
                              float *normal_xyz_out, void *stream);
int32_t mdh_contacts_device(mdh_renderer *r, int32_t n, const float *centre_xyz, const float *radius, const int32_t *kind_ixs,
                            int32_t n_kinds, float *dist_out, int32_t *index_out, float *normal_xyz_out, void *stream);

/* MESHING THE SCENE'S SURFACE, for a host's own rasteriser, physics, wireframe, OBJ export or baked distance volume: naive
 * surface nets over a regular grid, deterministic in values and in order (no atomics on the device).
 *
 * The grid: origin[3], cubic cells of `spacing` h > 0, cells[3] = (cx, cy, cz) cells, each >= 1; iso is the level.
 * D: n_kinds = 0 -- the whole scene as every pass sees it, through the space partition or the triangle BVH; n_kinds > 0 --
 * the exact scan of the listed kinds with the shaders' division, exactly as mdh_contacts takes kind_ixs and n_kinds (a host
 * lists Sphere and Box to mesh the objects without the room's walls).
 *
 * THE DEFINITION.  Every operation is one binary32 operation, unfused.
 *  1. Corner (i, j, k), 0 <= i <= cx and so on, lies at p_x = origin_x + (float) i * h -- one product, then one sum --
 *     likewise y and z.  Its value is v = fl (D (p) - iso): the bits mdh_contacts gives as dist at p with radius iso.  A
 *     corner is INSIDE iff v < 0; zero and NaN are outside.
 *  2. Cell (i, j, k), 0 <= i < cx and so on, has the corners c = 0 .. 7: bit 0 of c is the x offset, bit 1 the y offset,
 *     bit 2 the z offset.  A cell is ACTIVE iff some of its corners are inside and some are outside.
 *  3. The vertex of an active cell comes from its 12 edges in a fixed order: the outer loop over the axes a = x, y, z, the
 *     inner loop over e = 0 .. 3, where the two other axes in ascending order take the offsets e & 1 and e >> 1.  An edge
 *     CROSSES iff its endpoints v0 (offset 0 along a) and v1 differ in insideness; then t = v0 / (v0 - v1) and its local
 *     point q has t on axis a and the edge's offsets 0 or 1 on the other two.  s = s + q in that order from 0 over the m
 *     crossing edges, u = s / (float) m per component, and the world position is x = origin_x + ((float) i + u_x) * h: a
 *     sum, a product, a sum.
 *  4. Vertices are numbered by ascending cell id (k cy + j) cx + i.
 *  5. A vertex carries `index` and `normal`: the closest primitive at the vertex and its normal there, the bits
 *     mdh_contacts returns at that point for the same kind list.
 *  6. The grid edge along axis a from corner (i, j, k) emits a quad iff its a-coordinate is < cells[a], both other
 *     coordinates lie in 1 .. cells - 1 (all four cells round the edge exist) and its endpoints differ in insideness.
 *  7. With b = (a + 1) mod 3 and c = (a + 2) mod 3 the quad's four vertex ids are those of the cells at (b, c) offsets
 *     (-1, -1), (0, -1), (0, 0), (-1, 0) when the lower endpoint is inside -- the geometric normal then points along +a,
 *     out of the solid -- and in the reverse order otherwise.
 *  8. Quads are ordered by ascending key cornerid * 3 + a, cornerid = (k (cy + 1) + j) (cx + 1) + i.
 *
 * OUTPUTS, all optional but counts_out: positions_out and normals_out (3 floats a vertex), index_out (one int32 a vertex),
 * quads_out (4 int32 a quad), field_out ((cx + 1) (cy + 1) (cz + 1) corner values, x fastest: a baked distance volume),
 * counts_out[2] = the vertices and the quads FOUND, whatever the capacities.  The call writes the first min (found, capacity)
 * entries of each array and nothing behind them, and returns MDH_OK; a quad names the vertices by the ids they were found
 * with.  Capacity 0 with null arrays is a pure count.  With vertex_capacity > 0 at least one of the three vertex arrays is
 * given, with quad_capacity > 0 quads_out is; with capacity 0 none of them is.
 *
 * The contract is the ray queries' (mdh_raycast above): the query stream beside the frames in flight, pending
 * mdh_set_primitive, mdh_add_primitive and mdh_update_partitioning seen, nothing edited -- the probe-settle run and both
 * replays go on --, mdh_ray_query_time under MDH_OPT_TIMING from the first launch to the last.  Every refusal happens before
 * anything is launched:
 *   MDH_E_INVALID  a null renderer, origin, cells or counts_out; a cell count < 1; a non-finite origin, spacing or iso, or
 *                  spacing <= 0; |iso| above the scene's max_dist; a grid corner outside +-1024; a grid of more than
 *                  MDH_SURFACE_MAX_CORNERS corners; a negative capacity; an array with capacity 0, or a capacity > 0
 *                  without its array; n_kinds outside 0 .. MDH_MAX_KINDS or a kind index outside the scene's kinds
 *   MDH_E_STATE    a scene with a user-defined kind */
/* the grid's cap: 2^24 corners.  Every id the kernels form fits an int32 with room to spare (the largest, a quad's key
 * cornerid * 3 + 2, stays below 2^26), and the renderer's scratch -- a float a corner, an int32 a cell, two int32 per 256
 * corners -- stays below 129 MiB.  256^3 corners, a 255^3 grid of cells, is the largest cube. */
#define MDH_SURFACE_MAX_CORNERS 16777216
int32_t mdh_surface_mesh(mdh_renderer *r, const float *origin, float spacing, const int32_t *cells, float iso,
                         const int32_t *kind_ixs, int32_t n_kinds, int32_t vertex_capacity, int32_t quad_capacity,
                         float *positions_out, float *normals_out, int32_t *index_out, int32_t *quads_out, float *field_out,
                         int32_t *counts_out);
/* The same call for arrays the device addresses (origin, cells and kind_ixs stay the host's), under the contract of
 * mdh_raycast_device: asynchronous and ordered with `stream`, mdh_ray_query_wait is the host's wait, and where every array
 * lives and ends is checked before anything is launched (counts_out: 2 int32 the device addresses).  Nothing waits. */
int32_t mdh_surface_mesh_device(mdh_renderer *r, const float *origin, float spacing, const int32_t *cells, float iso,
                                const int32_t *kind_ixs, int32_t n_kinds, int32_t vertex_capacity, int32_t quad_capacity,
                                float *positions_out, float *normals_out, int32_t *index_out, int32_t *quads_out,
                                float *field_out, int32_t *counts_out, void *stream);

/* accumulated HIP-event time and launch count of one pass (MDH_OPT_TIMING) */
int32_t mdh_pass_time(mdh_renderer *r, int32_t pass, double *total_ms, int64_t *launches);
/* MDH_OPT_RADIANCE_REPLAY: the radiance passes launched since mdh_create that marched their rays (`plain`), marched them
 * and wrote the rays' records (`recording`), and read the records instead of marching (`replaying`).  Any pointer may be null. */
int32_t mdh_radiance_replay_stats(mdh_renderer *r, int64_t *plain, int64_t *recording, int64_t *replaying);
/* MDH_OPT_PROBE_SETTLE: the length of the run of consecutive irradiance passes of frames that changed no texel, under the
 * inputs that hold now (0 after any edit); the probe passes of frames that were not launched since mdh_create; the
 * texels the newest observed pass changed.  Reads what the device has reported so far and waits for nothing.  Any pointer
 * may be null. */
int32_t mdh_probe_settle_stats(mdh_renderer *r, int64_t *run, int64_t *skipped, int64_t *last_changed_texels);
/* MDH_OPT_SCREEN_REPLAY: the same count of the screen passes.  Any pointer may be null. */
int32_t mdh_screen_replay_stats(mdh_renderer *r, int64_t *plain, int64_t *recording, int64_t *replaying);
/* ... and the bytes of one pixel's record (32) */
int32_t mdh_screen_record_bytes(void);
int32_t mdh_reset_pass_times(mdh_renderer *r);

/* std140 layout queries = Scenes.Get_Primitives_Location / Get_Lights_Location
 * (madarch-scenes.adb:1435-1462) and Get_GPU_Type(...).Size */
int32_t mdh_scene_layout(mdh_renderer *r, int32_t is_light, int32_t kind_ix, int32_t *count_offset,
                         int32_t *array_offset, int32_t *stride, int32_t *element_size);
int32_t mdh_scene_buffer_size(mdh_renderer *r, int32_t *size, int32_t *total_light_count_offset);
/* raw std140 image of the scene uniform block (binding 1) for inspection */
int32_t mdh_read_scene_buffer(mdh_renderer *r, void *out, int32_t nbytes);
/* partition table as int32 [cell][n_prim_kinds counts + index_count indices] */
int32_t mdh_read_partitioning(mdh_renderer *r, int32_t *out, int32_t n_ints);
/* cells of the last Update_Partitioning whose candidate list overflowed Index_Count
 * (the reference prints "Warning : partition size too small", renderers.adb:593-598);
 * waits for that build */
int32_t mdh_partition_warnings(mdh_renderer *r);

/* MDH_OPT_TRIANGLE_BVH.  The builder by itself -- no renderer, no device: a top-down build (median of the centroids
 * along the longest axis, leaves of at most four triangles) over n_tris triangles of 9 floats (v1, v2, v3).
 *   nodes_out  the nodes in depth-first order as the kernels read them, 32 bytes each: float lo[3], int32 skip, float
 *              hi[3], int32 leaf -- skip = the node that follows this subtree (the root's is the node count), leaf = -1
 *              for an inner node (its first child is the next node), first * 8 + count for a leaf's range of perm_out.
 *              Room for max (1, 2 n_tris) nodes.
 *   perm_out   n_tris instance indices: the walked triangles in leaf order, then the always-evaluated list -- the
 *              triangles no geometric bound is trusted for (non-finite or huge vertices, tiny edges, slivers).
 *   delta_out  [0] = delta, [1] = rho: a subtree is skipped when its box is farther than closest (1 + rho) + delta.
 * Returns the length of the always-evaluated list (>= 0), or -MDH_E_INVALID.  The same input gives the same bytes. */
int32_t mdh_bvh_build(const float *tri_xyz, int32_t n_tris, void *nodes_out, int32_t *n_nodes, int32_t *perm_out, float *delta_out);
/* ... and the hierarchy of the renderer's committed scene (pending edits are committed first): node count, leaf count,
 * depth, length of the always-evaluated list; all 0 while the option is off or no Triangle kind is declared. */
int32_t mdh_triangle_bvh_info(mdh_renderer *r, int32_t *nodes, int32_t *leaves, int32_t *depth, int32_t *always);

const char *mdh_last_error(void);
const char *mdh_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MADARCH_HIP_H */
