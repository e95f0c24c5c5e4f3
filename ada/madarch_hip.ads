--  madarch_hip.ads -- thin Ada binding of include/madarch_hip.h (libmadarch_hip.so).
--
--  SOURCE ONLY: this pipeline has no Ada toolchain (no gnat1 / gprbuild), so this
--  unit has never been compiled here.  It is the binding a Madarch maintainer adds
--  next to madarch/madarch-renderers.ads; the replacement body that uses it is
--  ada/madarch-renderers.adb.  Link with -lmadarch_hip.

with Interfaces.C;
with Interfaces.C.Strings;
with System;

package Madarch_HIP is
   use Interfaces.C;

   subtype Status is int;   --  0 = ok; see the MDH_E_* codes of madarch_hip.h
   subtype Handle is System.Address;   --  mdh_renderer *

   OK             : constant Status := 0;
   E_Probe_Mismatch : constant Status := 2;   --  Program_Error, renderers.adb:63-65
   E_Index        : constant Status := 4;     --  Constraint_Error

   type Component is record
      Name : Strings.chars_ptr;
      Kind : int;           --  0 Vector3, 1 Float, 2 Int = Values.Value_Kind'Pos
   end record with Convention => C;
   type Component_Array is array (size_t range <>) of aliased Component
     with Convention => C;

   type Kind_Decl is record
      Name         : Strings.chars_ptr;
      Max_Count    : int;
      N_Components : int;
      Components   : System.Address;   --  const mdh_component *
      --  user-defined kinds (Primitives.Create): the Distance, Normal and Material
      --  expressions as MDH_X register programs; Null_Address / 0 for built-in kinds
      Dist_Code     : System.Address := System.Null_Address;   --  const int32_t *
      Dist_Len      : int := 0;
      Normal_Code   : System.Address := System.Null_Address;
      Normal_Len    : int := 0;
      Material_Code : System.Address := System.Null_Address;
      Material_Len  : int := 0;
   end record with Convention => C;
   type Kind_Decl_Array is array (size_t range <>) of aliased Kind_Decl
     with Convention => C;

   type Int3 is array (0 .. 2) of int with Convention => C;
   type Int2 is array (0 .. 1) of int with Convention => C;
   type Float3 is array (0 .. 2) of C_float with Convention => C;
   type Float9 is array (0 .. 8) of C_float with Convention => C;

   type Partitioning is record
      Enable, Index_Count, Border_Behavior : int;
      Grid_Dimensions : Int3;
      Grid_Spacing, Grid_Offset : Float3;
   end record with Convention => C;

   type Probe_Settings is record
      Radiance_Resolution, Irradiance_Resolution : int;
      Probe_Count     : Int2;
      Grid_Dimensions : Int3;
      Grid_Spacing    : Float3;
   end record with Convention => C;

   type Volumetrics is record
      Enabled               : int;
      Visibility_Resolution : Int3;
      Visibility_Step_Size  : C_float;
      Scattering_Resolution : Int2;
      Scattering_Step_Size  : C_float;
   end record with Convention => C;

   type Scene_Desc is record
      N_Prim_Kinds  : int;
      Prim_Kinds    : System.Address;
      N_Light_Kinds : int;
      Light_Kinds   : System.Address;
      Part          : Partitioning;
      Max_Dist      : C_float;
      Loop_Strategy : int;
   end record with Convention => C;

   function Create
     (Width, Height : int;
      Scene  : access constant Scene_Desc;
      Probes : access constant Probe_Settings;
      Vol    : access constant Volumetrics;
      Device : int;
      Result : access Handle) return Status
     with Import, Convention => C, External_Name => "mdh_create";

   function Destroy (R : Handle) return Status
     with Import, Convention => C, External_Name => "mdh_destroy";

   function Set_Material
     (R : Handle; Id0 : int; Albedo : access constant Float3;
      Metallic, Roughness : C_float) return Status
     with Import, Convention => C, External_Name => "mdh_set_material";

   function Set_Primitive
     (R : Handle; Kind_Ix, Index1 : int; Blob : System.Address; N_Bytes : int)
      return Status
     with Import, Convention => C, External_Name => "mdh_set_primitive";

   function Add_Primitive
     (R : Handle; Kind_Ix : int; Blob : System.Address; N_Bytes : int;
      Out_Count : access int) return Status
     with Import, Convention => C, External_Name => "mdh_add_primitive";

   function Set_Light
     (R : Handle; Index1, Light_Kind_Ix : int; Blob : System.Address;
      N_Bytes : int) return Status
     with Import, Convention => C, External_Name => "mdh_set_light";

   function Set_Camera_Position (R : Handle; P : access constant Float3)
      return Status
     with Import, Convention => C, External_Name => "mdh_set_camera_position";

   function Set_Camera_Orientation (R : Handle; M : access constant Float9)
      return Status
     with Import, Convention => C, External_Name => "mdh_set_camera_orientation";

   function Update_Partitioning (R : Handle; Method : int) return Status
     with Import, Convention => C, External_Name => "mdh_update_partitioning";

   function Render (R : Handle) return Status
     with Import, Convention => C, External_Name => "mdh_render";

   function Finish (R : Handle) return Status
     with Import, Convention => C, External_Name => "mdh_finish";

   --  MDH_OPT_* switches of madarch_hip.h.  Opt_Triangle_BVH: 1 = the triangles are walked through
   --  a bounding-volume hierarchy (the same bits; scenes with Partitioning => (Enable => False)
   --  and without user-defined kinds, Status 7 otherwise), 0 (default) = scanned one by one.
   Opt_Triangle_BVH : constant int := 20;
   --  Opt_Radiance_Replay: 1 (default) = probe rays' hits and cage visibility are replayed from
   --  per-ray records while the scene's geometry stands still (the same bits), 0 = marched every pass.
   Opt_Radiance_Replay : constant int := 21;
   --  Opt_Screen_Replay: 1 = the screen pass's hits and cage visibility are replayed from per-pixel
   --  records while camera and geometry stand still (the same bits), 0 (default) = marched every pass.
   Opt_Screen_Replay : constant int := 22;
   --  Opt_Probe_Settle: 1 (default) = a frame's radiance and irradiance passes are not launched once
   --  the probe atlases have stopped changing, the same bits; any edit launches them again; 0 = every frame
   Opt_Probe_Settle : constant int := 23;
   --  Opt_Ray_Stream_Refill: the device-array ray queries' wavefronts take new rays once this many of
   --  their 64 lanes are idle (1 .. 64; 64 = lock step; the same bits).  Opt_Ray_Stream_Groups: the
   --  workgroups such a query may launch, 0 (default) = as many as the device holds at once.
   Opt_Ray_Stream_Refill : constant int := 24;
   Opt_Ray_Stream_Groups : constant int := 25;
   --  Opt_Path_Frame_Compact: 1 = a round of an adaptive path-traced frame compacts the pixels
   --  still running; 0 (default, the measured one) = a retired pixel keeps its lane and idles.
   --  The same bits.
   Opt_Path_Frame_Compact : constant int := 26;

   function Set_Option (R : Handle; Option, Value : int) return Status
     with Import, Convention => C, External_Name => "mdh_set_option";

   function Read_Framebuffer (R : Handle; RGB_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_read_framebuffer";

   --  the window's RGBA8 pixels (Swap_Buffers, madarch-renderers.adb:320): enqueue, then fetch
   function Swap_Buffers (R : Handle) return Status
     with Import, Convention => C, External_Name => "mdh_swap_buffers";

   function Front_Buffer
     (R : Handle; RGBA : access System.Address; Swap_Count : access Interfaces.C.long) return Status
     with Import, Convention => C, External_Name => "mdh_front_buffer";

   function Eval_Distance_To
     (R : Handle; N : int; Points : System.Address; Kind_Ixs : System.Address;
      N_Kinds : int; Normals_Out, Dist_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_eval_distance_to";

   --  Ray queries (madarch_hip.h): the shaders' raycast, raycast_visibility and softshadows for
   --  N rays of the host's, on the device beside the frames in flight.  Org and Dir: 3 N floats,
   --  directions as given; every output of Raycast but Hit_Out may be Null_Address.  Scenes of
   --  built-in kinds only (Status 7 otherwise); they edit nothing.
   function Raycast
     (R : Handle; N : int; Org, Dir : System.Address;
      Hit_Out, Index_Out, T_Out, Steps_Out, Pos_Out, Normal_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_raycast";

   function Raycast_Visibility
     (R : Handle; N : int; Org, Dir, T_Max, Vis_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_raycast_visibility";

   function Softshadows
     (R : Handle; N : int; Org, Dir : System.Address; T_Min : C_float;
      T_Max : System.Address; K : C_float; Shadow_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_softshadows";

   --  The same three queries for arrays in memory the device addresses, asynchronous and ordered
   --  with Stream (a hipStream_t; Null_Address = the default stream): the kernel starts behind what
   --  Stream holds at the call, work given to Stream afterwards sees the answers, and the call does
   --  not wait.  A ray that is not finite (or whose T_Max exceeds the scene's max_dist) is not
   --  marched: Raycast answers Hit = -1, the other two NaN.  An array the device cannot address: Status 1.
   function Raycast_Device
     (R : Handle; N : int; Org, Dir : System.Address;
      Hit_Out, Index_Out, T_Out, Steps_Out, Pos_Out, Normal_Out : System.Address;
      Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_raycast_device";

   function Raycast_Visibility_Device
     (R : Handle; N : int; Org, Dir, T_Max, Vis_Out : System.Address;
      Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_raycast_visibility_device";

   function Softshadows_Device
     (R : Handle; N : int; Org, Dir : System.Address; T_Min : C_float;
      T_Max : System.Address; K : C_float; Shadow_Out : System.Address;
      Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_softshadows_device";

   --  blocks until every device query enqueued so far has ended
   function Ray_Query_Wait (R : Handle) return Status
     with Import, Convention => C, External_Name => "mdh_ray_query_wait";

   --  What a ray sees (madarch_hip.h): pixel_color_probes along N rays of the host's, through the
   --  pixel program of the screen pass.  Mode 0 (the fixed mode) or 2 (direct light times occlusion);
   --  Tone_Map 0 = the linear colour, 1 = the framebuffer's bits.  RGB_Out: 3 N floats, required;
   --  the other outputs may be Null_Address and count as in Read_Gbuffer.  Never any fog.  A ray that
   --  is not finite, starts beyond 1024 along an axis or has a direction component beyond 2 is not
   --  shaded: Status 1 for the batch of host arrays, NaN and Hit = -1 for that ray of device arrays.
   function Shade_Rays
     (R : Handle; N : int; Org, Dir : System.Address; Mode, Tone_Map : int;
      RGB_Out, Hit_Out, Index_Out, T_Out, Steps_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_shade_rays";

   function Shade_Rays_Device
     (R : Handle; N : int; Org, Dir : System.Address; Mode, Tone_Map : int;
      RGB_Out, Hit_Out, Index_Out, T_Out, Steps_Out : System.Address;
      Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_shade_rays_device";

   --  The rays of a Width x Height frame of the current camera, rows top first, 3 floats a ray:
   --  computed on the device by the screen pass's own functions, the frame's rays to the bit.
   function Camera_Rays
     (R : Handle; Width, Height : int; Org_Out, Dir_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_camera_rays";

   function Camera_Rays_Device
     (R : Handle; Width, Height : int; Org_Out, Dir_Out : System.Address;
      Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_camera_rays_device";

   --  What light arrives at a point the host owns (madarch_hip.h): pixel_color_probes from the hit on at
   --  N points that need not lie on a primitive.  Pos, Normal, View_Dir: 3 N floats each (View_Dir is the
   --  direction the point is seen along); Material_Ids: N ids as Add_Material returns them.  Mode 0,
   --  2, or 3 (Point_Irradiance: sample_irradiance alone; View_Dir and Material_Ids may be
   --  Null_Address, Tone_Map 0).  RGB_Out: 3 N floats.  A point that is not finite, lies beyond 1024,
   --  has a normal or view component beyond 1 or names no material is not shaded: Status 1 for the
   --  batch of host arrays, NaN for that point of device arrays.
   Point_Irradiance : constant int := 3;

   function Shade_Points
     (R : Handle; N : int; Pos, Normal, View_Dir, Material_Ids : System.Address;
      Mode, Tone_Map : int; RGB_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_shade_points";

   function Shade_Points_Device
     (R : Handle; N : int; Pos, Normal, View_Dir, Material_Ids : System.Address;
      Mode, Tone_Map : int; RGB_Out : System.Address; Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_shade_points_device";

   --  The material id of N primitive indices (the numbering of Read_Gbuffer and Raycast), -1 for -1
   --  and for an index no primitive has: a lookup on the host.
   function Primitive_Material
     (R : Handle; N : int; Index, Material_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_primitive_material";

   --  Ground truth for the probes: a path tracer along N rays of the host's (madarch_hip.h,
   --  mdh_path_trace).  RGB_Accum holds sums, in and out; ray I has id Id_First + I; Bounces 0 .. 6.
   function Path_Trace
     (R : Handle; N : int; Org, Dir : System.Address; Seed, Id_First : Interfaces.Unsigned_32;
      Sample_First, Sample_Count, Bounces : int;
      RGB_Accum, Hit_Out, Index_Out, T_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_path_trace";

   function Path_Trace_Device
     (R : Handle; N : int; Org, Dir : System.Address; Seed, Id_First : Interfaces.Unsigned_32;
      Sample_First, Sample_Count, Bounces : int;
      RGB_Accum, Hit_Out, Index_Out, T_Out : System.Address; Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_path_trace_device";

   --  The sampler by itself, on the host: no launch and no renderer.
   function Path_Scatter
     (N : int; Dir, Normal, Roughness : System.Address; Seed, Id_First : Interfaces.Unsigned_32;
      Sample, Bounce : int; Dir_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_path_scatter";

   --  A path-traced frame (madarch_hip.h, mdh_path_frame_begin): Path_Trace's estimator over the
   --  pixels of a frame of the camera, the sums kept on the device from call to call.  Begin
   --  captures the camera and fixes Seed, Bounces (0 .. 6) and Jitter (0 / 1); Accumulate adds the
   --  next Sample_Count samples and does not wait; Read is the resolve on the device, every output
   --  may be Null_Address; restarting after an edit of the scene is the caller's business.
   Path_Frame_Max_Pixels : constant int := 67_108_864;

   function Path_Frame_Begin
     (R : Handle; Width, Height : int; Seed : Interfaces.Unsigned_32; Bounces, Jitter : int)
      return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_begin";

   function Path_Frame_Accumulate (R : Handle; Sample_Count : int) return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_accumulate";

   function Path_Frame_Read
     (R : Handle; Tone_Map : int; RGB_Out, RGBA8_Out, Sums_Out : System.Address;
      Samples_Out : access int) return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_read";

   function Path_Frame_Read_Device
     (R : Handle; Tone_Map : int; RGB_Out, RGBA8_Out, Sums_Out : System.Address;
      Samples_Out : access int; Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_read_device";

   function Path_Frame_Rays
     (R : Handle; Sample : int; Org_Out, Dir_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_rays";

   function Path_Frame_Rays_Device
     (R : Handle; Sample : int; Org_Out, Dir_Out : System.Address; Stream : System.Address)
      return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_rays_device";

   function Path_Frame_Info
     (R : Handle; Width, Height, Samples, Bounces, Jitter : access int) return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_info";

   function Path_Frame_End (R : Handle) return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_end";

   --  The jitter by itself, on the host: no launch and no renderer.  UV_Out: 2 N floats.
   function Path_Pixel_Uv
     (Width, Height : int; Seed, Id_First : Interfaces.Unsigned_32; N, Sample, Jitter : int;
      UV_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_path_pixel_uv";

   --  An adaptive path-traced frame (madarch_hip.h, mdh_path_frame_begin_adaptive): beside its sums a
   --  pixel holds the count of its samples and two moments; Path_Frame_Accumulate is then one round
   --  for the pixels the stopping rule keeps running (evaluated at round boundaries only), and Read
   --  divides by the pixel's own count.  1 <= Min_Samples <= Max_Samples <= 2^24; Tolerance and
   --  Floor finite and >= 0.  A stopping rule on a biased variance estimate.
   function Path_Frame_Begin_Adaptive
     (R : Handle; Width, Height : int; Seed : Interfaces.Unsigned_32; Bounces, Jitter : int;
      Min_Samples, Max_Samples : int; Tolerance, Floor : C_float) return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_begin_adaptive";

   --  Count_Out: Width Height ints; Moments_Out: 2 Width Height floats; Active, Total_Samples:
   --  one 64-bit integer each.  Any address may be Null_Address.
   function Path_Frame_Stats
     (R : Handle; Count_Out, Moments_Out, Active, Total_Samples : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_stats";

   function Path_Frame_Stats_Device
     (R : Handle; Count_Out, Moments_Out, Active, Total_Samples : System.Address;
      Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_path_frame_stats_device";

   --  The rule by itself, on the host: no launch and no renderer.  Active_Out: N_Pixels bytes.
   function Path_Pixel_Active
     (N_Pixels : int; Count, M1, M2 : System.Address; Min_Samples, Max_Samples : int;
      Tolerance, Floor : C_float; Active_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_path_pixel_active";

   --  The lights' fog at N points and along N rays of the host's (madarch_hip.h,
   --  mdh_inscatter_points, mdh_inscatter_rays): the integrand of the visibility pass evaluated
   --  anywhere, and the scattering pass's serial sum along any ray.  F, Len_Out and Steps_Out may
   --  be Null_Address; March 0 or 1; at most Inscatter_Max_Steps steps of Step within max_dist.
   --  A point or ray that is not finite, or a T_Max outside 0 .. max_dist: Status 1 for the batch
   --  of host arrays, NaN and Steps = -1 for that one of device arrays.
   Inscatter_Max_Steps : constant int := 4096;

   function Inscatter_Points
     (R : Handle; N : int; Pos, Dir, F, RGB_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_inscatter_points";

   function Inscatter_Points_Device
     (R : Handle; N : int; Pos, Dir, F, RGB_Out : System.Address;
      Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_inscatter_points_device";

   function Inscatter_Rays
     (R : Handle; N : int; Org, Dir, T_Max : System.Address; March : int; Step : C_float;
      RGB_Out, Len_Out, Steps_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_inscatter_rays";

   function Inscatter_Rays_Device
     (R : Handle; N : int; Org, Dir, T_Max : System.Address; March : int; Step : C_float;
      RGB_Out, Len_Out, Steps_Out : System.Address; Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_inscatter_rays_device";

   --  Swept spheres and contacts for a host that owns moving bodies (madarch_hip.h,
   --  mdh_spherecast): Radius and T_Max may be Null_Address (0, the scene's max_dist);
   --  N_Kinds = 0 is the whole scene, otherwise Kind_Ixs lists the kinds to collide with
   function Spherecast
     (R : Handle; N : int; Org, Dir, Radius, T_Max, Kind_Ixs : System.Address; N_Kinds : int;
      Hit_Out, Index_Out, T_Out, Steps_Out, Pos_Out, Normal_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_spherecast";

   function Spherecast_Device
     (R : Handle; N : int; Org, Dir, Radius, T_Max, Kind_Ixs : System.Address; N_Kinds : int;
      Hit_Out, Index_Out, T_Out, Steps_Out, Pos_Out, Normal_Out : System.Address;
      Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_spherecast_device";

   function Contacts
     (R : Handle; N : int; Centre, Radius, Kind_Ixs : System.Address; N_Kinds : int;
      Dist_Out, Index_Out, Normal_Out : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_contacts";

   function Contacts_Device
     (R : Handle; N : int; Centre, Radius, Kind_Ixs : System.Address; N_Kinds : int;
      Dist_Out, Index_Out, Normal_Out : System.Address; Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_contacts_device";

   --  The scene's surface as a mesh: surface nets over a grid of Cells (3 ints) cubic cells of
   --  Spacing from Origin (3 floats) at level Iso (madarch_hip.h, mdh_surface_mesh, has the
   --  definition).  Every output but Counts_Out (2 ints: vertices and quads found) may be
   --  Null_Address with its capacity 0; N_Kinds as for Contacts
   Surface_Max_Corners : constant := 2 ** 24;

   function Surface_Mesh
     (R : Handle; Origin : System.Address; Spacing : C_float; Cells : System.Address;
      Iso : C_float; Kind_Ixs : System.Address; N_Kinds : int;
      Vertex_Capacity, Quad_Capacity : int;
      Positions_Out, Normals_Out, Index_Out, Quads_Out, Field_Out, Counts_Out : System.Address)
      return Status
     with Import, Convention => C, External_Name => "mdh_surface_mesh";

   function Surface_Mesh_Device
     (R : Handle; Origin : System.Address; Spacing : C_float; Cells : System.Address;
      Iso : C_float; Kind_Ixs : System.Address; N_Kinds : int;
      Vertex_Capacity, Quad_Capacity : int;
      Positions_Out, Normals_Out, Index_Out, Quads_Out, Field_Out, Counts_Out : System.Address;
      Stream : System.Address) return Status
     with Import, Convention => C, External_Name => "mdh_surface_mesh_device";

   --  One frame on the N GPUs of a node, one process per GPU (madarch_hip.h, mdh_comm_*):
   --  every process creates its Renderer on its own device, rank 0 makes a 128-byte id and
   --  hands it to the others (a file, an environment variable), all call Comm_Init, and
   --  from then on Render of every rank is one frame of the sharded schedule -- probe
   --  slices, RCCL all-gather inside the library, interleaved screen tiles.
   Comm_Id_Bytes : constant := 128;
   type Comm_Id is array (0 .. Comm_Id_Bytes - 1) of Interfaces.C.unsigned_char
     with Convention => C;

   function Comm_Unique_Id (Id_Out : access Comm_Id) return Status
     with Import, Convention => C, External_Name => "mdh_comm_unique_id";

   function Comm_Init
     (R : Handle; Id : access constant Comm_Id; Rank, World : int) return Status
     with Import, Convention => C, External_Name => "mdh_comm_init";

   function Comm_Destroy (R : Handle) return Status
     with Import, Convention => C, External_Name => "mdh_comm_destroy";

   function Comm_Barrier (R : Handle) return Status
     with Import, Convention => C, External_Name => "mdh_comm_barrier";

   --  the ranks' tiles of the last frame summed into Root's framebuffer (what its window shows)
   function Comm_Reduce_Framebuffer (R : Handle; Root : int) return Status
     with Import, Convention => C, External_Name => "mdh_comm_reduce_framebuffer";

   function Comm_Available return Status
     with Import, Convention => C, External_Name => "mdh_comm_available";

   function Comm_Abort (R : Handle) return Status
     with Import, Convention => C, External_Name => "mdh_comm_abort";

   --  The same sharded frame without a collective library (madarch_hip.h, mdh_peer_*): every
   --  rank exports 512 bytes of interprocess handles, the host hands all ranks' blobs to every
   --  rank, Peer_Init opens them, and Render's exchange is device-to-device copies ordered on
   --  the device.  One process per rank, one node; the form several ranks can run on ONE GPU.
   Peer_Blob_Bytes : constant := 512;
   type Peer_Blob is array (0 .. Peer_Blob_Bytes - 1) of Interfaces.C.unsigned_char
     with Convention => C;
   type Peer_Blobs is array (Natural range <>) of Peer_Blob
     with Convention => C;

   function Peer_Export (R : Handle; Blob_Out : access Peer_Blob) return Status
     with Import, Convention => C, External_Name => "mdh_peer_export";

   --  Blobs: the address of World blobs in rank order
   function Peer_Init
     (R : Handle; Blobs : System.Address; Rank, World : int) return Status
     with Import, Convention => C, External_Name => "mdh_peer_init";

   function Last_Error return Strings.chars_ptr
     with Import, Convention => C, External_Name => "mdh_last_error";
end Madarch_HIP;
