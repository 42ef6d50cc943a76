"""ctypes binding of libgpe.so (include/gpe.h).  No torch, no numpy arrays in the signatures:
plain pointers and sizes, exactly what a Rust `extern "C"` block would bind."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgpe.so")

GPE_OK = 0
GPE_ERR_INVALID_ARG = -1
GPE_ERR_HIP = -2
GPE_ERR_OOM = -3
GPE_ERR_STATE = -4
GPE_ERR_UNSUPPORTED = -5
GPE_ERR_NO_DEVICE = -6

MODE_COMPAT = 0
MODE_NATIVE = 1
FLAG_NATIVE_FORCE = 1
FLAG_SORT_EVERY_STEP = 2
FLAG_NATIVE_STATS = 4
FLAG_SAFE_SORT = 8
FLAG_COUNTING_SORT_TILES = 16
FLAG_XCD_EIGHTHS = 64
FLAG_NO_HALF_TILES = 128
FLAG_SHARD_OVERLAP = 256
FLAG_FUSED_HISTOGRAMS = 512
FLAG_GUARD_ALLOCS = 1024
FLAG_HASH_INDEX64 = 2048
FLAG_EVENT_SCOPES = 4096
FLAG_GENERAL_RADII = 8192
PIPELINE_COMPAT, PIPELINE_NATIVE = 0, 1
(REASON_NONE, REASON_MODE_COMPAT, REASON_NO_PARTICLES, REASON_OUT_OF_BOX, REASON_GRID_TOO_WIDE,
 REASON_TABLE_TOO_LARGE, REASON_DENSE_WINDOWS) = range(7)
STEP_RESORT = 1

UNUSED_CELL_ID = 0xFFFFFFFF
MAX_CELLS_PER_OBJECT = 4
COUNTING_CHUNK_SIZE = 4

# gpe_array
POS, PREV, RADIUS, HOME_CELL_IDS, PARTICLE_IDS, CELL_IDS, OBJECT_IDS, COLLISION_CELLS, \
    NUM_COLLISION_CELLS, CHUNK_OBJ_COUNT, INDIRECT_ARGS, ORDER_KEYS, UIDS = range(13)
UID_ABSENT = 0xFFFFFFFF
RAY_MISS = 0xFFFFFFFF
NEAREST_NONE = 0xFFFFFFFF
TRACERS_MAX = 65536
TRACER_POS, TRACER_PREV, TRACER_INDEX = 1, 2, 4
TRACERS_CONSUME = 1
MONITOR_CONSUME = 1
NEAREST_MAX_M = 64
COLLIDERS_MAX = 4096
BONDS_MAX, BOND_MAX_DEGREE, BOND_ITER_MAX = 4194304, 1024, 32
BOND_ANCHOR, BOND_BROKEN = 1, 2
BENDS_MAX, BEND_MAX_DEGREE, BEND_ITER_MAX = 4194304, 1024, 32
AREAS_MAX, AREA_MAX_MEMBERS, AREA_MEMBERS_MAX, AREA_MAX_DEGREE, AREA_ITER_MAX = 4194304, 4096, 16777216, 64, 32
BODIES_MAX, BODY_MAX_MEMBERS, BODY_MEMBERS_MAX = 1048576, 4096, 16777216
BODY_BROKEN = 1
FIELDS_MAX = 4096
FIELD_EVERYWHERE, FIELD_CIRCLE, FIELD_BOX = 0, 1, 2
FIELD_UNIFORM, FIELD_RADIAL, FIELD_VORTEX, FIELD_DRAG = 0, 1, 2, 3
FALLOFF_NONE, FALLOFF_LINEAR = 0, 1
MOVERS_MAX = 1024
MOVER_LINEAR, MOVER_ROTATE = 0, 1
SURFACES_OF_COLLIDERS, SURFACES_OF_MOVERS = 0, 1
SURFACE_PLAIN = 1
SWEEP_OFF, SWEEP_ON = 0, 1
BOND_SOLVER_JACOBI, BOND_SOLVER_COLOURED = 0, 1
BOND_COLOURS_MAX = 64
BEND_SOLVER_JACOBI, BEND_SOLVER_COLOURED = 0, 1
BEND_COLOURS_MAX = 64
EDIT_BY_INDEX, EDIT_BY_UID = 0, 1
CLUSTER_BY_INDEX, CLUSTER_BY_UID = 0, 1
VEL_ADD, VEL_SET, VEL_SCALE = 0, 1, 2
SPAWN_SEPARATE, SPAWN_INSIDE_WORLD, SPAWN_DRY_RUN = 1, 2, 4
SPAWN_ADDED, SPAWN_BLOCKED_BY_PARTICLE, SPAWN_BLOCKED_BY_CANDIDATE, SPAWN_OUTSIDE_WORLD = 0, 1, 2, 3


class GpeConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32),
        ("world_width", C.c_float), ("world_height", C.c_float),
        ("gravity_x", C.c_float), ("gravity_y", C.c_float),
        ("cell_size_multiplier", C.c_float), ("stiffness", C.c_float),
        ("mouse_strength", C.c_float), ("mode", C.c_uint32), ("profiling", C.c_uint32),
        ("flags", C.c_uint32), ("guard_canary", C.c_uint32), ("guard_poison", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class GpePipelineInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pipeline", C.c_uint32), ("reason", C.c_uint32),
                ("sort_passes", C.c_uint32), ("native_steps", C.c_uint64), ("compat_steps", C.c_uint64),
                ("native_sorts", C.c_uint64), ("window_max", C.c_uint32), ("roster_stamp", C.c_uint32),
                ("overflow_tiles", C.c_uint32), ("overflow_subtiles", C.c_uint32), ("overflow_spills", C.c_uint32),
                ("arena_slots", C.c_uint32)]


class GpePipelineInfoUniform(C.Structure):
    """gpe_pipeline_info as it stands; GpePipelineInfo is the shorter layout up to arena_slots, which the library still
    serves by its struct_size."""
    _fields_ = GpePipelineInfo._fields_ + [("uniform_radius", C.c_uint32)]


class GpeTiming(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("total_ms", C.c_double), ("calls", C.c_uint64)]


class GpeTraceEvent(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("start_ms", C.c_double), ("duration_ms", C.c_double)]


class GpeShardPlan(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("rank", C.c_uint32), ("world_size", C.c_uint32), ("n_slots", C.c_uint32),
        ("blocks_x", C.c_int32), ("blocks_y", C.c_int32),
        ("d_owner_of_block", C.c_void_p), ("d_dest_mask_of_block", C.c_void_p),
        ("slot_rank", C.c_uint32 * 9),
        ("send_off", C.c_uint32 * 9), ("send_cap_mig", C.c_uint32 * 9), ("send_cap_gho", C.c_uint32 * 9),
        ("recv_off", C.c_uint32 * 9), ("recv_cap_mig", C.c_uint32 * 9), ("recv_cap_gho", C.c_uint32 * 9),
        ("d_send", C.c_void_p), ("d_recv", C.c_void_p),
        ("own_x0", C.c_int32), ("own_y0", C.c_int32), ("own_x1", C.c_int32), ("own_y1", C.c_int32),
    ]


# gpe_shard_transport_fn
SHARD_TRANSPORT_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
COMM_ID_BYTES = 128
SHARD_MAX_RANKS = 26
REDUCE_SUM, REDUCE_MAX = 0, 1


class GpeShardLayout(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("world_size", C.c_uint32), ("px", C.c_uint32), ("py", C.c_uint32),
        ("world_width", C.c_float), ("world_height", C.c_float), ("cell_size", C.c_float),
        ("cells_x", C.c_int32), ("cells_y", C.c_int32), ("blocks_x", C.c_int32), ("blocks_y", C.c_int32),
        ("xcuts", C.c_int32 * 27), ("ycuts", C.c_int32 * 27),
    ]


# gpe_shard_collectives.all_reduce_u32 / .all_to_all_u32
ALL_REDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p)
ALL_TO_ALL_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p,
                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p)


class GpeShardCollectives(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("user", C.c_void_p),
                ("all_reduce_u32", ALL_REDUCE_FN), ("all_to_all_u32", ALL_TO_ALL_FN)]


class GpeShardStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("recuts", C.c_uint32), ("resorts", C.c_uint64), ("steps", C.c_uint64),
                ("n_owned", C.c_uint64), ("n_ghost", C.c_uint64), ("n_neighbours", C.c_uint32), ("transport", C.c_uint32)]


class GpeQueryResult(C.Structure):
    """gpe_query_result: in struct_size / capacity, out count; every array pointer may be NULL."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("capacity", C.c_uint64), ("count", C.c_uint64),
                ("index", C.POINTER(C.c_uint32)), ("uid", C.POINTER(C.c_uint32)), ("pos_xy", C.POINTER(C.c_float)),
                ("prev_xy", C.POINTER(C.c_float)), ("radius", C.POINTER(C.c_float))]


class GpeContactResult(C.Structure):
    """gpe_contact_result: in struct_size / capacity, out count; every array pointer may be NULL (degree: u32[gpe_len])."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("capacity", C.c_uint64), ("count", C.c_uint64),
                ("index_a", C.POINTER(C.c_uint32)), ("index_b", C.POINTER(C.c_uint32)), ("uid_a", C.POINTER(C.c_uint32)),
                ("uid_b", C.POINTER(C.c_uint32)), ("overlap", C.POINTER(C.c_float)), ("degree", C.POINTER(C.c_uint32))]


class GpeClusterResult(C.Structure):
    """gpe_cluster_result: in struct_size, out count / largest_size / largest_label; every array pointer may be NULL
    (each u32[gpe_len])."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("count", C.c_uint64),
                ("largest_size", C.c_uint32), ("largest_label", C.c_uint32), ("label", C.POINTER(C.c_uint32)),
                ("size", C.POINTER(C.c_uint32)), ("label_uid", C.POINTER(C.c_uint32))]


class GpeRayCast(C.Structure):
    """gpe_ray_cast: in struct_size / flags / k and the endpoint arrays, out hits; every output pointer may be NULL."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("k", C.c_uint64),
                ("from_xy", C.POINTER(C.c_float)), ("to_xy", C.POINTER(C.c_float)), ("index", C.POINTER(C.c_uint32)),
                ("uid", C.POINTER(C.c_uint32)), ("t", C.POINTER(C.c_float)), ("pos_xy", C.POINTER(C.c_float)),
                ("radius", C.POINTER(C.c_float)), ("hits", C.c_uint64)]


class GpeNearestQuery(C.Structure):
    """gpe_nearest_query: in struct_size / flags / k / point_xy / m / max_distance, out found; every output pointer may be
    NULL (count u32[k], the others m slots per point)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("k", C.c_uint64),
                ("point_xy", C.POINTER(C.c_float)), ("m", C.c_uint32), ("max_distance", C.c_float),
                ("count", C.POINTER(C.c_uint32)), ("index", C.POINTER(C.c_uint32)), ("uid", C.POINTER(C.c_uint32)),
                ("dist2", C.POINTER(C.c_float)), ("pos_xy", C.POINTER(C.c_float)), ("radius", C.POINTER(C.c_float)),
                ("found", C.c_uint64)]


class GpeTracerConfig(C.Structure):
    """gpe_tracer_config: all in -- fields (TRACER_*), the k uids to follow, a frame after every every-th step, a ring of
    `frames` frames."""
    _fields_ = [("struct_size", C.c_uint32), ("fields", C.c_uint32), ("k", C.c_uint64),
                ("uids", C.POINTER(C.c_uint32)), ("every", C.c_uint64), ("frames", C.c_uint64)]


class GpeTracerFrames(C.Structure):
    """gpe_tracer_frames: in struct_size / flags / capacity, out count / recorded; every array may be NULL (step
    u64[capacity], pos_xy / prev_xy f32[capacity * k * 2], index u32[capacity * k])."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("capacity", C.c_uint64),
                ("count", C.c_uint64), ("recorded", C.c_uint64), ("step", C.POINTER(C.c_uint64)),
                ("pos_xy", C.POINTER(C.c_float)), ("prev_xy", C.POINTER(C.c_float)), ("index", C.POINTER(C.c_uint32))]


class GpeMeasures(C.Structure):
    """gpe_measures: one record of the run monitor, 120 bytes (all out)."""
    _fields_ = [("step", C.c_uint64), ("n", C.c_uint64), ("irregular", C.c_uint64), ("moving", C.c_uint64),
                ("outside", C.c_uint64), ("sum_x", C.c_double), ("sum_y", C.c_double), ("sum_vx", C.c_double),
                ("sum_vy", C.c_double), ("sum_v2", C.c_double), ("min_x", C.c_float), ("min_y", C.c_float),
                ("max_x", C.c_float), ("max_y", C.c_float), ("max_v2", C.c_float), ("max_v2_index", C.c_uint32),
                ("max_v2_uid", C.c_uint32), ("first_irregular", C.c_uint32), ("first_irregular_uid", C.c_uint32),
                ("reserved", C.c_uint32)]


class GpeMonitorConfig(C.Structure):
    """gpe_monitor_config: all in -- flags 0, a frame after every every-th step, a ring of `frames` records, the moving
    threshold rest_speed (displacement per step)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("every", C.c_uint64), ("frames", C.c_uint64),
                ("rest_speed", C.c_float), ("reserved", C.c_uint32)]


class GpeMonitorFrames(C.Structure):
    """gpe_monitor_frames: in struct_size / flags / capacity, out count / recorded; frames (gpe_measures[capacity]) may
    be NULL."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("capacity", C.c_uint64), ("count", C.c_uint64),
                ("recorded", C.c_uint64), ("frames", C.POINTER(GpeMeasures))]


class GpeCollider(C.Structure):
    """gpe_collider: a capsule, the segment a -> b thickened by radius; flags 0.  24 bytes."""
    _fields_ = [("ax", C.c_float), ("ay", C.c_float), ("bx", C.c_float), ("by", C.c_float), ("radius", C.c_float),
                ("flags", C.c_uint32)]


class GpeCollidersInfo(C.Structure):
    """gpe_colliders_info: in struct_size; out the colliders set, the passes run and particles moved since the last
    gpe_set_colliders, the lookup grid in use and its (cell, collider) entries."""
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_uint32), ("passes", C.c_uint64), ("pushed", C.c_uint64),
                ("grid_x", C.c_uint32), ("grid_y", C.c_uint32), ("list_entries", C.c_uint64)]


class GpeSweepInfo(C.Structure):
    """gpe_sweep_info: in struct_size; out the sweep mode of the static colliders' pass, the swept passes run since the
    last gpe_set_collider_sweep, the particles swept (winner at 0 < t < 1) and stopped by them.  32 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_uint32), ("passes", C.c_uint64), ("swept", C.c_uint64),
                ("stopped", C.c_uint64)]


class GpeBond(C.Structure):
    """gpe_bond: particle uid_a tied to particle uid_b, or (BOND_ANCHOR, uid_b = UID_ABSENT) to the point (anchor_x,
    anchor_y), at rest_length.  32 bytes."""
    _fields_ = [("uid_a", C.c_uint32), ("uid_b", C.c_uint32), ("rest_length", C.c_float), ("stiffness", C.c_float),
                ("max_length", C.c_float), ("flags", C.c_uint32), ("anchor_x", C.c_float), ("anchor_y", C.c_float)]


class GpeBondsInfo(C.Structure):
    """gpe_bonds_info: in struct_size; out the relaxations per pass, the bonds set and the distinct uids they name, and
    since the last gpe_set_bonds the passes run, the bonds not broken / broken and the times the uids were looked up."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("k", C.c_uint64), ("nodes", C.c_uint64),
                ("passes", C.c_uint64), ("live", C.c_uint64), ("broken", C.c_uint64), ("resolves", C.c_uint64)]


class GpeBondSolverInfo(C.Structure):
    """gpe_bond_solver_info: in struct_size; out the bonds' solver mode, the colours of the set held and the bonds of the
    fullest one, the launch form of the last coloured pass (0 none yet, 1 per colour, 2 one workgroup), the node count
    up to which form 2 is taken, the coloured passes run since the last gpe_set_bond_solver.  32 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_uint32), ("colours", C.c_uint32),
                ("largest_colour", C.c_uint32), ("form", C.c_uint32), ("lds_nodes_max", C.c_uint32),
                ("passes", C.c_uint64)]


class GpeBendSolverInfo(C.Structure):
    """gpe_bend_solver_info: in struct_size; out the bends' solver mode, the colours of the set held and the bends of the
    fullest one, the launch form of the last coloured pass (0 none yet, 1 per colour, 2 one workgroup), the node count
    up to which form 2 is taken, the coloured passes run since the last gpe_set_bend_solver.  32 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_uint32), ("colours", C.c_uint32),
                ("largest_colour", C.c_uint32), ("form", C.c_uint32), ("lds_nodes_max", C.c_uint32),
                ("passes", C.c_uint64)]


class GpeBend(C.Structure):
    """gpe_bend: the angle at the hinge uid_b from (uid_a - uid_b) to (uid_c - uid_b) held at the rest angle
    (rest_cos, rest_sin).  32 bytes."""
    _fields_ = [("uid_a", C.c_uint32), ("uid_b", C.c_uint32), ("uid_c", C.c_uint32), ("rest_cos", C.c_float),
                ("rest_sin", C.c_float), ("stiffness", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class GpeBendsInfo(C.Structure):
    """gpe_bends_info: in struct_size; out the relaxations per pass, the bends set and the distinct uids they name, and
    since the last gpe_set_bends the passes run and the times the uids were looked up.  40 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("k", C.c_uint64), ("nodes", C.c_uint64),
                ("passes", C.c_uint64), ("resolves", C.c_uint64)]


class GpeArea(C.Structure):
    """gpe_area: members [first, first + count) of the set's member uids, in order around a closed polygon, keep the
    signed rest_area.  24 bytes."""
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("rest_area", C.c_float), ("stiffness", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class GpeAreasInfo(C.Structure):
    """gpe_areas_info: in struct_size; out the relaxations per pass, the loops set, their members and the distinct uids
    they name, and since the last gpe_set_areas the passes run and the times the uids were looked up.  48 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("k", C.c_uint64), ("members", C.c_uint64),
                ("nodes", C.c_uint64), ("passes", C.c_uint64), ("resolves", C.c_uint64)]


class GpeBody(C.Structure):
    """gpe_body: members [first, first + count) of the set's member arrays keep their rest shape.  24 bytes."""
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("stiffness", C.c_float), ("break_distance", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class GpeBodiesInfo(C.Structure):
    """gpe_bodies_info: in struct_size; out the bodies set and their members, and since the last gpe_set_bodies the
    passes run, the bodies not broken / broken and the times the uids were looked up."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("k", C.c_uint64), ("members", C.c_uint64),
                ("passes", C.c_uint64), ("live", C.c_uint64), ("broken", C.c_uint64), ("resolves", C.c_uint64)]


class GpeField(C.Structure):
    """gpe_field: a region (shape; x0, y0, x1, y1) and what it does to the particles whose centre lies in it (kind,
    falloff; the pole px, py; the acceleration fx, fy; strength; reach); flags 0.  56 bytes."""
    _fields_ = [("shape", C.c_uint32), ("kind", C.c_uint32), ("falloff", C.c_uint32), ("flags", C.c_uint32),
                ("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float),
                ("px", C.c_float), ("py", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("strength", C.c_float), ("reach", C.c_float)]


class GpeFieldsInfo(C.Structure):
    """gpe_fields_info: in struct_size; out the fields set, the passes run and the particles whose prev they wrote since
    the last gpe_set_fields, the lookup grid in use and its (cell, field) entries."""
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_uint32), ("passes", C.c_uint64), ("touched", C.c_uint64),
                ("grid_x", C.c_uint32), ("grid_y", C.c_uint32), ("list_entries", C.c_uint64)]


class GpeMover(C.Structure):
    """gpe_mover: a capsule at rest (ax, ay, bx, by, radius) and its motion: kind LINEAR (vx, vy; travel) or ROTATE (the
    pivot px, py; omega); flags and reserved 0.  56 bytes."""
    _fields_ = [("ax", C.c_float), ("ay", C.c_float), ("bx", C.c_float), ("by", C.c_float), ("radius", C.c_float),
                ("kind", C.c_uint32), ("vx", C.c_float), ("vy", C.c_float), ("travel", C.c_float),
                ("px", C.c_float), ("py", C.c_float), ("omega", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class GpeMoverPose(C.Structure):
    """gpe_mover_pose: the posed capsule and the motion state (LINEAR: g, sgn; ROTATE: c, s).  24 bytes."""
    _fields_ = [("ax", C.c_float), ("ay", C.c_float), ("bx", C.c_float), ("by", C.c_float), ("q0", C.c_float), ("q1", C.c_float)]


class GpeMoversInfo(C.Structure):
    """gpe_movers_info: in struct_size; out the movers set, the passes run and particles moved since the last
    gpe_set_movers, the lookup grid of the last build, its mask words per cell and the (cell, mover) bits it set."""
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_uint32), ("passes", C.c_uint64), ("pushed", C.c_uint64),
                ("grid_x", C.c_uint32), ("grid_y", C.c_uint32), ("mask_words", C.c_uint32), ("reserved", C.c_uint32),
                ("listed", C.c_uint64)]


class GpeSurface(C.Structure):
    """gpe_surface: the material of one static collider or mover: restitution in [0, 1], friction >= 0, flags
    (SURFACE_PLAIN: this obstacle keeps the plain rule), reserved 0.  16 bytes."""
    _fields_ = [("restitution", C.c_float), ("friction", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class GpeParticleEdit(C.Structure):
    """gpe_particle_edit: in struct_size / key_kind / k / keys and the field arrays (each may be NULL), out edited."""
    _fields_ = [("struct_size", C.c_uint32), ("key_kind", C.c_uint32), ("k", C.c_uint64),
                ("keys", C.POINTER(C.c_uint32)), ("pos_xy", C.POINTER(C.c_float)), ("prev_xy", C.POINTER(C.c_float)),
                ("radius", C.POINTER(C.c_float)), ("edited", C.c_uint64)]


class GpeParticleSpawn(C.Structure):
    """gpe_particle_spawn: in struct_size / flags / k and the candidate arrays, out verdict (may be NULL) and added."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("k", C.c_uint64),
                ("pos_xy", C.POINTER(C.c_float)), ("radius", C.POINTER(C.c_float)), ("verdict", C.POINTER(C.c_uint8)),
                ("added", C.c_uint64)]


GUARD_MAX_ZONES = 8
GUARD_FRONT, GUARD_REAR = 0, 1


class GpeGuardZone(C.Structure):
    """gpe_guard_zone: one damaged red zone (offsets: front relative to the payload's first byte, rear to its end)."""
    _fields_ = [("tag", C.c_char * 32), ("side", C.c_uint32), ("first_word", C.c_uint32),
                ("first_offset", C.c_int64), ("last_offset", C.c_int64), ("payload_bytes", C.c_uint64)]


class GpeGuardReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("damaged", C.c_uint32), ("listed", C.c_uint32),
                ("allocations", C.c_uint32), ("zones", GpeGuardZone * GUARD_MAX_ZONES)]


class GpeError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("gpe status %d: %s" % (status, message))
        self.status = status


# every symbol include/gpe.h declares: (name, restype, argtypes)
_VP, _U64, _U32, _I32, _F = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_float
SYMBOLS = [
    ("gpe_abi_version", _U32, []),
    ("gpe_config_default", _I32, [C.POINTER(GpeConfig)]),
    ("gpe_create", _I32, [C.POINTER(GpeConfig), C.POINTER(_VP)]),
    ("gpe_destroy", _I32, [_VP]),
    ("gpe_last_error", C.c_char_p, [_VP]),
    ("gpe_set_particles", _I32, [_VP, _VP, _VP, _VP, _U64]),
    ("gpe_add_particles", _I32, [_VP, _VP, _VP, _U64]),
    ("gpe_remove_particles", _I32, [_VP, _VP, _U64, C.POINTER(_U64)]),
    ("gpe_remove_particles_in_circle", _I32, [_VP, _F, _F, _F, C.POINTER(_U64)]),
    ("gpe_enable_uids", _I32, [_VP, _I32]),
    ("gpe_set_uids", _I32, [_VP, _VP, _U64]),
    ("gpe_next_uid", _I32, [_VP, C.POINTER(_U64)]),
    ("gpe_set_next_uid", _I32, [_VP, _U64]),
    ("gpe_find_uids", _I32, [_VP, _VP, _U64, _VP, _VP, _VP, _VP]),
    ("gpe_remove_particles_by_uid", _I32, [_VP, _VP, _U64, C.POINTER(_U64)]),
    ("gpe_tracers_begin", _I32, [_VP, C.POINTER(GpeTracerConfig)]),
    ("gpe_tracers_sample", _I32, [_VP]),
    ("gpe_tracers_read", _I32, [_VP, C.POINTER(GpeTracerFrames)]),
    ("gpe_tracers_end", _I32, [_VP]),
    ("gpe_measure", _I32, [_VP, _F, C.POINTER(GpeMeasures)]),
    ("gpe_monitor_begin", _I32, [_VP, C.POINTER(GpeMonitorConfig)]),
    ("gpe_monitor_sample", _I32, [_VP]),
    ("gpe_monitor_read", _I32, [_VP, C.POINTER(GpeMonitorFrames)]),
    ("gpe_monitor_end", _I32, [_VP]),
    ("gpe_set_colliders", _I32, [_VP, C.POINTER(GpeCollider), _U64]),
    ("gpe_get_colliders", _I32, [_VP, C.POINTER(GpeCollider), _U64, C.POINTER(_U64)]),
    ("gpe_apply_colliders", _I32, [_VP]),
    ("gpe_get_colliders_info", _I32, [_VP, C.POINTER(GpeCollidersInfo)]),
    ("gpe_set_collider_sweep", _I32, [_VP, _U32]),
    ("gpe_get_collider_sweep", _I32, [_VP, C.POINTER(_U32)]),
    ("gpe_get_sweep_info", _I32, [_VP, C.POINTER(GpeSweepInfo)]),
    ("gpe_set_mover_sweep", _I32, [_VP, _U32]),
    ("gpe_get_mover_sweep", _I32, [_VP, C.POINTER(_U32)]),
    ("gpe_get_mover_sweep_info", _I32, [_VP, C.POINTER(GpeSweepInfo)]),
    ("gpe_set_bonds", _I32, [_VP, C.POINTER(GpeBond), _U64, C.c_uint32]),
    ("gpe_get_bonds", _I32, [_VP, C.POINTER(GpeBond), C.POINTER(C.c_uint8), _U64, C.POINTER(_U64)]),
    ("gpe_apply_bonds", _I32, [_VP]),
    ("gpe_get_bonds_info", _I32, [_VP, C.POINTER(GpeBondsInfo)]),
    ("gpe_set_bond_solver", _I32, [_VP, _U32]),
    ("gpe_get_bond_solver", _I32, [_VP, C.POINTER(_U32)]),
    ("gpe_get_bond_solver_info", _I32, [_VP, C.POINTER(GpeBondSolverInfo)]),
    ("gpe_set_bends", _I32, [_VP, C.POINTER(GpeBend), _U64, C.c_uint32]),
    ("gpe_get_bends", _I32, [_VP, C.POINTER(GpeBend), _U64, C.POINTER(_U64)]),
    ("gpe_apply_bends", _I32, [_VP]),
    ("gpe_get_bends_info", _I32, [_VP, C.POINTER(GpeBendsInfo)]),
    ("gpe_set_bend_solver", _I32, [_VP, _U32]),
    ("gpe_get_bend_solver", _I32, [_VP, C.POINTER(_U32)]),
    ("gpe_get_bend_solver_info", _I32, [_VP, C.POINTER(GpeBendSolverInfo)]),
    ("gpe_set_areas", _I32, [_VP, C.POINTER(GpeArea), _U64, C.POINTER(C.c_uint32), _U64, C.c_uint32]),
    ("gpe_get_areas", _I32, [_VP, C.POINTER(GpeArea), _U64, C.POINTER(_U64), C.POINTER(C.c_uint32), _U64, C.POINTER(_U64)]),
    ("gpe_apply_areas", _I32, [_VP]),
    ("gpe_get_areas_info", _I32, [_VP, C.POINTER(GpeAreasInfo)]),
    ("gpe_get_area_values", _I32, [_VP, C.POINTER(C.c_float), _U64, C.POINTER(_U64)]),
    ("gpe_set_area_targets", _I32, [_VP, _U64, _U64, C.POINTER(C.c_float)]),
    ("gpe_set_bodies", _I32, [_VP, C.POINTER(GpeBody), _U64, C.POINTER(C.c_uint32), C.POINTER(C.c_float), _U64]),
    ("gpe_get_bodies", _I32, [_VP, C.POINTER(GpeBody), C.POINTER(C.c_uint8), _U64, C.POINTER(_U64),
                              C.POINTER(C.c_uint32), C.POINTER(C.c_float), _U64, C.POINTER(_U64)]),
    ("gpe_apply_bodies", _I32, [_VP]),
    ("gpe_get_body_poses", _I32, [_VP, C.POINTER(C.c_float), _U64, C.POINTER(_U64)]),
    ("gpe_get_bodies_info", _I32, [_VP, C.POINTER(GpeBodiesInfo)]),
    ("gpe_set_fields", _I32, [_VP, C.POINTER(GpeField), _U64]),
    ("gpe_get_fields", _I32, [_VP, C.POINTER(GpeField), _U64, C.POINTER(_U64)]),
    ("gpe_apply_fields", _I32, [_VP, _F]),
    ("gpe_get_fields_info", _I32, [_VP, C.POINTER(GpeFieldsInfo)]),
    ("gpe_set_movers", _I32, [_VP, C.POINTER(GpeMover), _U64]),
    ("gpe_get_movers", _I32, [_VP, C.POINTER(GpeMover), _U64, C.POINTER(_U64)]),
    ("gpe_get_mover_poses", _I32, [_VP, C.POINTER(GpeMoverPose), _U64, C.POINTER(_U64)]),
    ("gpe_set_mover_poses", _I32, [_VP, C.POINTER(GpeMoverPose), _U64]),
    ("gpe_apply_movers", _I32, [_VP, _F]),
    ("gpe_get_movers_info", _I32, [_VP, C.POINTER(GpeMoversInfo)]),
    ("gpe_set_surfaces", _I32, [_VP, _U32, C.POINTER(GpeSurface), _U64]),
    ("gpe_get_surfaces", _I32, [_VP, _U32, C.POINTER(GpeSurface), _U64, C.POINTER(_U64)]),
    ("gpe_query_circle", _I32, [_VP, _F, _F, _F, C.POINTER(GpeQueryResult)]),
    ("gpe_query_box", _I32, [_VP, _F, _F, _F, _F, C.POINTER(GpeQueryResult)]),
    ("gpe_pick", _I32, [_VP, _F, _F, C.POINTER(GpeQueryResult)]),
    ("gpe_query_contacts", _I32, [_VP, C.POINTER(GpeContactResult)]),
    ("gpe_query_clusters", _I32, [_VP, C.POINTER(GpeClusterResult)]),
    ("gpe_query_cluster_of", _I32, [_VP, _U32, _U32, C.POINTER(GpeQueryResult)]),
    ("gpe_cast_rays", _I32, [_VP, C.POINTER(GpeRayCast)]),
    ("gpe_query_segment", _I32, [_VP, _F, _F, _F, _F, C.POINTER(GpeQueryResult)]),
    ("gpe_query_nearest", _I32, [_VP, C.POINTER(GpeNearestQuery)]),
    ("gpe_edit_particles", _I32, [_VP, C.POINTER(GpeParticleEdit)]),
    ("gpe_add_particles_free", _I32, [_VP, C.POINTER(GpeParticleSpawn)]),
    ("gpe_kick_circle", _I32, [_VP, _F, _F, _F, _U32, _F, _F, C.POINTER(_U64)]),
    ("gpe_kick_box", _I32, [_VP, _F, _F, _F, _F, _U32, _F, _F, C.POINTER(_U64)]),
    ("gpe_len", _I32, [_VP, C.POINTER(_U64)]),
    ("gpe_max_radius", _I32, [_VP, C.POINTER(_F)]),
    ("gpe_morton_resort", _I32, [_VP]),
    ("gpe_integrate", _I32, [_VP, _F]),
    ("gpe_set_mouse", _I32, [_VP, _I32, _F, _F]),
    ("gpe_set_world", _I32, [_VP, _F, _F]),
    ("gpe_set_gravity", _I32, [_VP, _F, _F]),
    ("gpe_world", _I32, [_VP, C.POINTER(_F), C.POINTER(_F)]),
    ("gpe_gravity", _I32, [_VP, C.POINTER(_F), C.POINTER(_F)]),
    ("gpe_mouse", _I32, [_VP, C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F)]),
    ("gpe_compute_cell_size", _F, [_F]),
    ("gpe_grid_set_max_radius", _I32, [_VP, _F]),
    ("gpe_cell_size", _I32, [_VP, C.POINTER(_F)]),
    ("gpe_grid_max_radius", _I32, [_VP, C.POINTER(_F)]),
    ("gpe_grid_build", _I32, [_VP]),
    ("gpe_grid_sort", _I32, [_VP]),
    ("gpe_grid_update", _I32, [_VP]),
    ("gpe_solve_collisions", _I32, [_VP]),
    ("gpe_build_collision_cells", _I32, [_VP]),
    ("gpe_step", _I32, [_VP, _F, _U32]),
    ("gpe_run", _I32, [_VP, _F, _U64, _U64, _I32]),
    ("gpe_sync", _I32, [_VP]),
    ("gpe_set_mode", _I32, [_VP, _U32]),
    ("gpe_get_pipeline_info", _I32, [_VP, _VP]),                 # (either layout of gpe_pipeline_info)
    ("gpe_download", _I32, [_VP, C.c_int, _VP, _U64]),
    ("gpe_array_bytes", _I32, [_VP, C.c_int, C.POINTER(_U64)]),
    ("gpe_device_ptr", _I32, [_VP, C.c_int, C.POINTER(_VP), C.POINTER(_U64)]),
    ("gpe_buffer_alloc", _I32, [_VP, _U64, C.POINTER(_VP)]),
    ("gpe_buffer_free", _I32, [_VP, _VP]),
    ("gpe_buffer_upload", _I32, [_VP, _VP, _VP, _U64]),
    ("gpe_buffer_download", _I32, [_VP, _VP, _VP, _U64]),
    ("gpe_sort_pairs_u32", _I32, [_VP, _VP, _VP, _U64]),
    ("gpe_sort_histogram_u32", _I32, [_VP, _VP, _U64, _U32, _VP]),
    ("gpe_sort_scatter_pass_u32", _I32, [_VP, _VP, _VP, _VP, _VP, _U64, _U32]),
    ("gpe_inclusive_scan_u32", _I32, [_VP, _VP, _U64]),
    ("gpe_reserve", _I32, [_VP, _U64]),
    ("gpe_capacity", _I32, [_VP, C.POINTER(_U64)]),
    ("gpe_set_counts", _I32, [_VP, _U64, _U64]),
    ("gpe_use_order_keys", _I32, [_VP, _I32]),
    ("gpe_set_active_cells", _I32, [_VP, _I32, _I32, _I32, _I32]),
    ("gpe_stream_handle", _I32, [_VP, C.POINTER(_VP)]),
    ("gpe_set_stream", _I32, [_VP, _VP]),
    ("gpe_refresh", _I32, [_VP]),
    ("gpe_shard_classify", _I32, [_VP, _VP, _VP, _I32, _I32, _U32, _VP, _VP, _VP, _U64]),
    ("gpe_shard_configure", _I32, [_VP, C.POINTER(GpeShardPlan)]),
    ("gpe_shard_begin", _I32, [_VP]),
    ("gpe_shard_unpack", _I32, [_VP]),
    ("gpe_shard_step", _I32, [_VP, _F]),
    ("gpe_shard_peek", _I32, [_VP, C.POINTER(_U64), C.POINTER(_U64)]),
    ("gpe_shard_counts", _I32, [_VP, C.POINTER(_U64), C.POINTER(_U64), _I32]),
    ("gpe_comm_probe", _I32, []),
    ("gpe_comm_unique_id", _I32, [_VP]),
    ("gpe_shard_comm_init", _I32, [_VP, _VP, _U32, _U32]),
    ("gpe_shard_comm_attach", _I32, [_VP, _VP]),
    ("gpe_shard_comm_destroy", _I32, [_VP]),
    ("gpe_shard_set_transport", _I32, [_VP, _VP, _VP]),
    ("gpe_shard_exchange", _I32, [_VP]),
    ("gpe_shard_run", _I32, [_VP, _F, _U64]),
    ("gpe_shard_layout_build", _I32, [_F, _F, _F, _U32, _U32, _U32, _VP, _VP, C.POINTER(GpeShardLayout)]),
    ("gpe_shard_layout_owner_of", _I32, [C.POINTER(GpeShardLayout), _VP, _U64, _VP]),
    ("gpe_shard_quantile_cuts", _I32, [_VP, _U32, _U32, _U32, _VP]),
    ("gpe_shard_set_collectives", _I32, [_VP, C.POINTER(GpeShardCollectives)]),
    ("gpe_local_group_create", _I32, [_U32, C.POINTER(_VP)]),
    ("gpe_local_group_destroy", _I32, [_VP]),
    ("gpe_local_group_join", _I32, [_VP, _VP, _U32]),
    ("gpe_local_group_abort", _I32, [_VP]),
    ("gpe_shard_set_particles", _I32, [_VP, _VP, _VP, _VP, _VP, _U64, _U64]),
    ("gpe_shard_setup", _I32, [_VP, C.POINTER(GpeShardLayout), _U32, _F]),
    ("gpe_shard_get_layout", _I32, [_VP, C.POINTER(GpeShardLayout)]),
    ("gpe_shard_resort", _I32, [_VP]),
    ("gpe_shard_recut", _I32, [_VP, _F, C.POINTER(_I32)]),
    ("gpe_shard_run_scheduled", _I32, [_VP, _F, _U64, _U64, _I32]),
    ("gpe_shard_download_owned", _I32, [_VP, _VP, _VP, _VP, _U64, C.POINTER(_U64)]),
    ("gpe_shard_get_stats", _I32, [_VP, C.POINTER(GpeShardStats)]),
    ("gpe_set_profiling", _I32, [_VP, _U32]),
    ("gpe_reset_timings", _I32, [_VP]),
    ("gpe_get_timings", _I32, [_VP, C.POINTER(GpeTiming), C.POINTER(_U32)]),
    ("gpe_get_trace", _I32, [_VP, C.POINTER(GpeTraceEvent), C.POINTER(_U32)]),
    ("gpe_guard_check", _I32, [_VP, C.POINTER(GpeGuardReport)]),
    ("gpe_guard_registry", _I32, [_VP, C.c_char_p, _U64, C.POINTER(_U64)]),
]

_lib = None


def load():
    """dlopen libgpe.so.  There is no CPU or pure-Python fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python gpu-physics-engine_amd/build.py` "
            "(or __graft_entry__.build()); the HIP extension is the only implementation" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(status, ctx=None):
    if status != GPE_OK:
        msg = load().gpe_last_error(ctx)
        raise GpeError(status, msg.decode() if msg else "")
