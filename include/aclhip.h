/* aclhip.h -- C ABI of the MI355X-native batched ACL clip decompressor (libaclhip.so).
 *
 * This is the drop-in boundary for the reference's decompression path. The reference has no ABI: its
 * boundary is the inlined C++ template surface of acl::decompression_context<Settings>
 * (/root/reference/includes/acl/decompression/decompress.h:76-201). Each entry point below names the
 * reference interface it replaces; acl_amd/csrc/aclhip.hpp rebuilds the reference's C++ surface on top
 * of these calls, and INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no HIP or torch types: device pointers are `void*`/typed pointers into HBM of the context's
 *     device, streams are passed as `void*` (a hipStream_t; NULL = the default stream);
 *   - every function returns an aclhip_status and never throws; decompress calls are asynchronous and
 *     stream ordered (the reference's calls are synchronous CPU code);
 *   - a context owns device copies of registered clips; the caller owns instance lists and pose buffers;
 *   - a pose is `num_tracks` records of 48 bytes, the reference's rtm::qvvf:
 *     rotation xyzw | translation xyz, 0 | scale xyz, 0   (core/impl/debug_track_writer.h:61-62,172-192).
 */
#ifndef ACLHIP_H
#define ACLHIP_H

#include <stdint.h>

#if defined(__cplusplus)
extern "C" {
#endif

#define ACLHIP_VERSION_MAJOR 0
#define ACLHIP_VERSION_MINOR 1

typedef enum aclhip_status
{
	ACLHIP_OK = 0,
	ACLHIP_ERROR_INVALID_ARGUMENT = 1,
	ACLHIP_ERROR_INVALID_CLIP = 2,			/* compressed_tracks::is_valid() would fail (core/impl/compressed_tracks.impl.h:278-301) */
	ACLHIP_ERROR_UNSUPPORTED_FORMAT = 3,	/* an unknown track type or rotation format; tables beyond the limits registration states */
	ACLHIP_ERROR_UNKNOWN_CLIP = 4,
	ACLHIP_ERROR_OUT_OF_MEMORY = 5,
	ACLHIP_ERROR_DEVICE = 6,				/* a HIP call failed, see aclhip_last_error_message */
	ACLHIP_ERROR_NO_DEVICE = 7,
	ACLHIP_ERROR_UNKNOWN_DATABASE = 8,
	ACLHIP_ERROR_NOT_IN_DATABASE = 9,
	ACLHIP_ERROR_NO_METADATA = 10			/* the blob does not carry the optional metadata that was asked for */
} aclhip_status;

/* acl::sample_rounding_policy (core/sample_rounding_policy.h) */
typedef enum aclhip_rounding_policy
{
	ACLHIP_ROUND_NONE = 0,
	ACLHIP_ROUND_FLOOR = 1,
	ACLHIP_ROUND_CEIL = 2,
	ACLHIP_ROUND_NEAREST = 3,
	ACLHIP_ROUND_PER_TRACK = 4
} aclhip_rounding_policy;

/* acl::sample_looping_policy (core/sample_looping_policy.h) */
typedef enum aclhip_looping_policy
{
	ACLHIP_LOOP_CLAMP = 0,
	ACLHIP_LOOP_WRAP = 1,
	ACLHIP_LOOP_AS_COMPRESSED = 2
} aclhip_looping_policy;

/* acl::rotation_normalization_policy_t (decompression/decompression_settings.h:50-62) */
typedef enum aclhip_normalization_policy
{
	ACLHIP_NORMALIZE_NEVER = 0,
	ACLHIP_NORMALIZE_LERP_ONLY = 1,			/* default_transform_decompression_settings */
	ACLHIP_NORMALIZE_ALWAYS = 2
} aclhip_normalization_policy;

/* acl::default_sub_track_mode (core/track_writer.h:49-74) */
typedef enum aclhip_default_mode
{
	ACLHIP_DEFAULT_SKIPPED = 0,				/* default sub-tracks are not written, the caller pre-filled the pose buffer */
	ACLHIP_DEFAULT_CONSTANT = 1,			/* one value for every default sub-track (identity / 0 / 1 when no value is given) */
	ACLHIP_DEFAULT_VARIABLE = 2,			/* per track value, e.g. the bind pose */
	ACLHIP_DEFAULT_LEGACY = 3,				/* scale only: the clip's default scale bit (ACL 2.0 behaviour) */
	ACLHIP_DEFAULT_BIND_POSE = 4			/* not in the reference: variable, with every clip's OWN table -- track_desc_transformf::default_value of each track,
											 * read from the blob's optional track descriptions at registration (compressed_tracks::get_track_description,
											 * core/impl/compressed_tracks.impl.h:214-275); the identity for clips that carry none. What a caller of the
											 * reference does by hand: get_track_description() per track into a debug_track_writer_variable_defaults */
} aclhip_default_mode;

typedef struct aclhip_context aclhip_context;
typedef uint32_t aclhip_clip;				/* handle returned by aclhip_register_clip */
typedef uint32_t aclhip_database;			/* handle returned by aclhip_register_database */

#define ACLHIP_INVALID_HANDLE 0xFFFFFFFFu

/* What decompression_settings + track_writer select at compile time in the reference
 * (decompression/decompression_settings.h:74-166, core/track_writer.h:82-216), as a run time struct.
 * aclhip_default_params() fills in default_transform_decompression_settings + the track_writer defaults. */
typedef struct aclhip_decompress_params
{
	uint8_t rounding_policy;				/* aclhip_rounding_policy given to seek() for every instance (unless per-instance policies are supplied) */
	uint8_t looping_policy;					/* aclhip_looping_policy, decompression_context::set_looping_policy() */
	uint8_t normalization;					/* aclhip_normalization_policy, get_rotation_normalization_policy() */
	uint8_t per_track_rounding;				/* is_per_track_rounding_supported() */
	uint8_t default_rotation_mode;			/* aclhip_default_mode, track_writer::get_default_rotation_mode() */
	uint8_t default_translation_mode;
	uint8_t default_scale_mode;
	uint8_t reserved0;
	const float* default_values;			/* DEVICE pointer or NULL. CONSTANT: 12 floats; VARIABLE: max num_tracks * 12 floats (qvv per track) */
	const uint8_t* track_rounding_policies;	/* DEVICE pointer or NULL: track_writer::get_rounding_policy() per track, used when seeking with PER_TRACK */
	const uint8_t* instance_rounding_policies;	/* DEVICE pointer or NULL: one aclhip_rounding_policy per instance, overrides rounding_policy */
	const uint8_t* instance_looping_policies;	/* DEVICE pointer or NULL: one aclhip_looping_policy per instance, overrides looping_policy --
												 * decompression_context::set_looping_policy() belongs to ONE context = one instance (decompress.h:149) */
	/* track_writer::get_rounding_policy(policy, track_index) (core/track_writer.h:97) belongs to the writer of ONE pose as well: M tables
	 * of track_rounding_stride bytes each (a table = what track_rounding_policies is: one aclhip_rounding_policy per track), instance i
	 * seeks and decodes with table instance_rounding_tables[i] (< M, the caller's table: not checked). Overrides track_rounding_policies.
	 * Both or neither; per instance arrays are indexed by the caller's instance index (aclhip_output_desc). */
	const uint8_t* track_rounding_table;		/* DEVICE pointer or NULL */
	const uint8_t* instance_rounding_tables;	/* DEVICE pointer or NULL: one table index per instance */
	uint32_t track_rounding_stride;				/* bytes from one table to the next (>= tracks of the largest clip of the batch) */
	uint32_t flags;								/* ACLHIP_DECODE_* (reserved1 until ABI 6: aclhip_default_params has always zeroed it) */
} aclhip_decompress_params;

/* aclhip_decompress_params::flags.
 * ACLHIP_DECODE_FAST: opt in, per launch. The default kernels follow the reference's x86 arithmetic one IEEE operation at a time and are bit
 * exact with it (math/quatf.h:135-211); north_star's bar is 1e-5. With this flag an animated ROTATION is computed with the hardware's 1 ulp
 * square root / reciprocal square root and fused multiply-adds: every rotation component stays within 2e-6 of the default kernels'
 * (tests/test_gpu_fast_decode.py asserts it over every instance of the BASELINE.json batches and the corpus); the x, y, z of every sample
 * (the range expansions are never fused), constant and default sub-tracks, translations and scales are bit identical. Taken by the plain
 * decode (aclhip_decompress_tracks_batch / _rows / _list with the QVV48 layout and the track_writer defaults); launches with other settings
 * or an output descriptor keep the exact kernels, as do per track rounding policies and aclhip_decompress_track_batch (its variant never
 * measured faster than the exact kernel and was removed: the flag is accepted there and changes nothing). What it removes is vector
 * instructions of poses of several windows (the 300-bone rig: 4 % of them) -- worth 2 % of the launch while both kernels ran at 7 waves
 * per SIMD and nothing since the exact kernel fits 8 (190.7 against 190.8 us); a one-window batch sits on its write stream either way. */
#define ACLHIP_DECODE_FAST 1u

/* Where a decoded pose goes and what of it: the run time form of the OUTPUT side of the track_writer protocol
 * (core/track_writer.h:161-216). A writer decides per sub-track kind whether it wants it at all -- skip_all_rotations /
 * skip_all_translations / skip_all_scales (:181-183) -- and the writer's own pose type decides how wide a bone is: the
 * reference's debug writer stores rtm::qvvf (48 bytes, core/impl/debug_track_writer.h:61-62), its benchmark counts
 * sizeof(rtm::quatf) + 2 * sizeof(rtm::float3f) = 40 bytes per bone (tools/acl_decompressor/sources/benchmark.cpp:146), engines
 * that ignore scale keep 32. The decode sits on the HBM write roofline, so bytes per pose are poses per second. */
typedef enum aclhip_pose_layout
{
	ACLHIP_LAYOUT_QVV48 = 0,				/* per track: rotation xyzw | translation xyz 0 | scale xyz 0 (rtm::qvvf), the default */
	ACLHIP_LAYOUT_QVV40 = 1,				/* per track: rotation xyzw | translation xyz | scale xyz, 10 packed floats */
	ACLHIP_LAYOUT_QV32 = 2					/* per track: rotation xyzw | translation xyz 0; scales are not written (implies skip_scales) */
} aclhip_pose_layout;

typedef struct aclhip_output_desc
{
	uint32_t layout;						/* aclhip_pose_layout */
	uint8_t skip_rotations;					/* track_writer::skip_all_rotations(): no rotation is written, its bytes in the pose buffer are left untouched */
	uint8_t skip_translations;				/* track_writer::skip_all_translations() */
	uint8_t skip_scales;					/* track_writer::skip_all_scales() */
	uint8_t reserved0;
	const uint32_t* rows;					/* DEVICE pointer or NULL: pose of instance i goes to row rows[i] (distinct) instead of row i */
	const uint8_t* skip_tracks;				/* DEVICE pointer or NULL: track_writer::skip_track_rotation / _translation / _scale(track_index)
											 * (core/track_writer.h:189-191) for the whole launch: one byte per track (as many as the largest clip of
											 * the batch has tracks), bit 0 / 1 / 2 set = the track's rotation / translation / scale is skipped -- not
											 * written, its bytes in the pose buffer are left untouched (an LOD that drops finger bones) */
	/* Per INSTANCE writer decisions (ABI 5). In the reference the track_writer belongs to ONE decompress_tracks call, i.e. to one pose:
	 * skip_track_rotation / _translation / _scale(track_index) (core/track_writer.h:189-191) are per character. A crowd with per
	 * character LODs is ONE launch here:
	 *   mask_table + instance_masks   M skip masks of mask_stride bytes each (a mask = what skip_tracks is: one byte per track, bit 0 / 1 / 2 =
	 *                                 rotation / translation / scale skipped); instance i uses mask instance_masks[i] (< M, not checked: the
	 *                                 caller's table). Overrides skip_tracks.
	 *   instance_track_counts         instance i stores only its first instance_track_counts[i] tracks (the LOD most engines use: bones are
	 *                                 ordered by importance); nothing beyond is decoded, DMA'd or written -- on a kernel bound by its
	 *                                 writes, bytes not written are poses per second. A count above the clip's track count changes nothing.
	 * Every per instance array of this struct and of aclhip_decompress_params is indexed by the CALLER's instance index (instance lists:
	 * the index in the list handed to aclhip_instance_list_set_clips, whatever order the library decodes in). */
	const uint8_t* mask_table;				/* DEVICE pointer or NULL */
	const uint8_t* instance_masks;			/* DEVICE pointer or NULL: one mask index per instance; needs mask_table */
	const uint32_t* instance_track_counts;	/* DEVICE pointer or NULL */
	uint32_t mask_stride;					/* bytes from one mask of mask_table to the next (>= tracks of the largest clip of the batch) */
	uint32_t reserved1;
} aclhip_output_desc;

typedef struct aclhip_clip_info
{
	uint32_t num_tracks;
	uint32_t num_samples;
	float sample_rate;
	float duration;							/* compressed_tracks::get_finite_duration(as_compressed) */
	uint32_t num_segments;
	uint32_t has_scale;
	uint32_t looping_policy;				/* compressed_tracks::get_looping_policy() */
	uint32_t compressed_size;				/* compressed_tracks::get_size() */
	uint32_t hash;							/* compressed_tracks::get_hash() */
	uint32_t num_animated_sub_tracks;		/* rotations + translations + scales */
	uint32_t has_database;
	uint32_t has_stripped_keyframes;
	uint32_t track_type;					/* acl::track_type8 (core/track_types.h:51-68): 12 qvvf; 0..4 float1f, float2f, float3f, float4f, vector4f */
	uint32_t num_components;				/* floats per sample of a track: 12 for qvvf (one qvv record), 1..4 for scalar track lists */
} aclhip_clip_info;

/* ---- library / context ------------------------------------------------------------------------ */

const char* aclhip_status_string(aclhip_status status);

/* Message of the last failing call made on the CALLING thread (empty string when none); `context` is not used to find it. */
const char* aclhip_last_error_message(const aclhip_context* context);

/* The layouts of the structs in this header as a number: bumped whenever one of them changes (3: aclhip_output_desc::skip_tracks;
 * 4: aclhip_pose_consumers::num_blend_clips, flags, blend_clips, blend_sample_times, blend_weights;
 * 5: aclhip_decompress_params::instance_looping_policies, track_rounding_table, instance_rounding_tables, track_rounding_stride, aclhip_output_desc::mask_table, instance_masks, instance_track_counts, mask_stride;
 * 6: ACLHIP_DEFAULT_BIND_POSE, aclhip_clip_metadata_info; ACLHIP_ERROR_UNSUPPORTED_FORMAT no longer covers the full-precision formats;
 * track maps -- aclhip_track_map_info, aclhip_track_mapping and their entry points -- were ADDED without a bump: no existing struct or
 * entry point changed shape, so a caller built against the earlier header 6 hands over nothing of another shape; the same goes for
 * skeletons -- aclhip_skeleton_info, aclhip_pose_mapping and their entry points -- and for the pose error measure -- aclhip_pose_error,
 * aclhip_pose_error_worst, aclhip_pose_error_desc and aclhip_measure_pose_error_batch -- and for the matrix object space --
 * aclhip_matrix_layout, aclhip_pose_matrices_desc, aclhip_error_metric, aclhip_pose_matrices_batch and
 * aclhip_measure_pose_error_metric_batch -- and for the skinning palettes -- aclhip_skin_info, aclhip_palette_layout,
 * aclhip_skinning_desc, the four skin entry points and aclhip_skinning_matrices_batch -- and for raw track arrays --
 * aclhip_raw_tracks_info, aclhip_raw_sample_desc, the four raw track entry points and aclhip_sample_raw_tracks_batch -- and for raw
 * scalar track arrays and the scalar track error -- aclhip_raw_scalar_tracks_info, aclhip_scalar_error_desc, the four raw scalar track
 * entry points, aclhip_sample_raw_scalar_tracks_batch, aclhip_sample_raw_scalar_track_batch and aclhip_measure_scalar_error_batch -- and
 * for the scalar compressor -- aclhip_scalar_compress_desc, aclhip_compress_result, aclhip_scalar_compress_bound,
 * aclhip_scalar_compress_workspace_bytes and aclhip_compress_raw_scalar_tracks_batch -- and for the raw-format transform compressor --
 * aclhip_transform_compress_desc, aclhip_transform_compress_bound, aclhip_transform_compress_workspace_bytes and
 * aclhip_compress_raw_tracks_batch -- and for the drop-w transform compressor -- aclhip_compress_tracks_desc,
 * aclhip_compress_tracks_workspace_bytes and aclhip_compress_tracks_batch -- and for the variable formats at given bit rates --
 * aclhip_compress_variable_desc, aclhip_variable_compress_num_segments, aclhip_variable_compress_bound,
 * aclhip_compress_variable_workspace_bytes and aclhip_compress_tracks_variable_batch -- and for their bit rate search --
 * aclhip_find_bit_rates_desc, aclhip_find_bit_rates_workspace_bytes and aclhip_find_bit_rates_batch -- and for the transform
 * compressors with the error metric as an argument -- aclhip_compress_tracks_metric_batch,
 * aclhip_compress_tracks_variable_metric_batch and aclhip_find_bit_rates_metric_batch).
 * A caller compiled against another header would hand over structs of another shape; aclhip_abi_version() says what the LIBRARY was
 * built with, and the C++ mirror (aclhip.hpp) refuses to create a context when the two differ. */
#define ACLHIP_ABI_VERSION 6u
uint32_t aclhip_abi_version(void);

/* Creates a context bound to HIP device `device_index` (replaces nothing in the reference: contexts there are
 * 128 byte stack objects, decompression/impl/decompression_context.transform.h:53-116). */
aclhip_status aclhip_create(int device_index, aclhip_context** out_context);
void aclhip_destroy(aclhip_context* context);

void aclhip_default_params(aclhip_decompress_params* out_params);

/* ---- clips ------------------------------------------------------------------------------------ */

/* Replaces decompression_context::initialize(const compressed_tracks&) (decompress.h:103; impl/decompress.impl.h:66-83;
 * initialize_v0 impl/decompression.transform.h:84-132): validates the blob like compressed_tracks::is_valid(check_hash)
 * and copies it, unchanged and 16 byte aligned with tail padding, into HBM together with derived lookup tables.
 * `compressed_tracks` is a HOST pointer to `size` bytes; the caller may free it as soon as the call returns. */
aclhip_status aclhip_register_clip(aclhip_context* context, const void* compressed_tracks, uint64_t size, int check_hash, aclhip_clip* out_clip);

/* Replaces decompression_context::reset() / the end of the blob's lifetime. Like every call that registers, replaces or retires
 * something (clips, hierarchies, databases) it never synchronizes the device and nobody waits: decodes that were ENQUEUED before the
 * call, on any stream this context has launched on, still decode the clip (its record in the device table is cleared behind them, on
 * a stream of the context's own); launches that execute later refuse the handle (counted, poses untouched); the clip's memory and its
 * handle are recycled when both have happened. The caller's side of the contract is the reference's: do not enqueue a decode of a
 * clip after its unregistration. */
aclhip_status aclhip_unregister_clip(aclhip_context* context, aclhip_clip clip);

/* The context remembers every stream it has launched on (retired clips, hierarchies and databases wait for the work enqueued on
 * them). Call this BEFORE destroying a stream the context has launched on: it waits for that stream's work (hipStreamSynchronize)
 * and forgets the stream. A destroyed stream the context still remembers is detected when its next event cannot be recorded, but
 * using a stale handle is undefined behaviour by HIP's rules -- this call is the defined way. */
aclhip_status aclhip_forget_stream(aclhip_context* context, void* stream);

/* Counters of the stream ordered lifetime management, for tests and tools: out_stats[0] clips registered, [1] clips unregistered,
 * [2] retired items whose memory has been recycled, [3] retired items still waiting for work in flight, [4] capacity of the clip
 * table in records, [5] 1 when the table grows inside a reserved address range (it never moves either way), [6] its device
 * address, [7] streams the context has launched on. out_stats holds 8 values. */
aclhip_status aclhip_get_lifetime_stats(aclhip_context* context, uint64_t* out_stats);

aclhip_status aclhip_get_clip_info(const aclhip_context* context, aclhip_clip clip, aclhip_clip_info* out_info);

/* The optional metadata a blob may carry behind its compressed data (compression_metadata_settings, compression_settings.h:84-120): read and
 * bounds checked once, at registration. Replaces compressed_tracks::get_parent_track_index / get_track_description
 * (core/impl/compressed_tracks.impl.h:175-275) for registered clips. */
typedef struct aclhip_clip_metadata_info
{
	uint32_t has_metadata;					/* tracks_header::get_has_metadata() */
	uint32_t has_parent_track_indices;		/* ... and the section is stored (and lies inside the blob) */
	uint32_t has_track_descriptions;
	uint32_t has_track_names;
	uint32_t has_track_list_name;
	uint32_t has_contributing_error;
} aclhip_clip_metadata_info;
aclhip_status aclhip_get_clip_metadata_info(const aclhip_context* context, aclhip_clip clip, aclhip_clip_metadata_info* out_info);

/* Host only (no context, no device), on a blob that need not be registered -- where the reference's accessors live: which optional sections
 * the blob stores and, for the arrays that are not null (capacity = the tracks they hold), get_parent_track_index / get_track_description of
 * every track as the two calls below return them. Sections that are not stored leave their arrays untouched. */
aclhip_status aclhip_read_clip_metadata(const void* compressed_tracks, uint64_t size, aclhip_clip_metadata_info* out_info, uint32_t* out_parent_indices,
	float* out_default_values, float* out_precisions, float* out_shell_distances, uint32_t capacity);

/* compressed_tracks::get_parent_track_index for every track (ACLHIP_NO_PARENT = k_invalid_track_index); `capacity` entries are available at
 * out_parent_indices and must cover the clip's tracks. ACLHIP_ERROR_NO_METADATA when the blob does not store them. */
aclhip_status aclhip_get_clip_parent_indices(const aclhip_context* context, aclhip_clip clip, uint32_t* out_parent_indices, uint32_t capacity);

/* compressed_tracks::get_track_description(track, track_desc_transformf&) for every track: default_value as 12 floats per track (rotation
 * xyzw | translation xyz 0 | scale xyz 0: a row of aclhip_decompress_params::default_values), and -- both optional -- precision and
 * shell_distance. `capacity` = tracks the arrays hold. ACLHIP_ERROR_NO_METADATA when the blob does not store descriptions. */
aclhip_status aclhip_get_clip_track_descriptions(const aclhip_context* context, aclhip_clip clip, float* out_default_values, float* out_precisions, float* out_shell_distances, uint32_t capacity);

/* Replaces compressed_tracks::is_valid(check_hash) (core/impl/compressed_tracks.impl.h:278-301) as a host only call (no context,
 * no device): everything aclhip_register_clip checks before it uploads -- tag, version, hash, every header offset, sub-track
 * classes against counts, bit widths against the per segment pose size, stored keyframes inside the buffer. `out_message`
 * (optional) receives the reason, like error_result::c_str(). The reference only checks alignment, tag, version and hash; the
 * rest is here because the device reads through these offsets -- and, since round 5, because a buffer that is accepted has to decode to
 * the SAME poses here and in the reference: also refused are blobs the reference's decoder and these kernels would read differently
 * (a segment whose sample range claims keyframes that overlap the next segment's data; a stripped segment that does not keep its first
 * and last sample; segment start indices without their 0xFFFFFFFF end or that the reference's guess-and-scan lookup would resolve to
 * other segments; per segment rotation / translation bit sizes and constant sample counts that disagree with the sub-track types;
 * section offsets that are not 4 byte aligned). Everything the reference's compressor writes passes. */
aclhip_status aclhip_check_clip(const void* compressed_tracks, uint64_t size, int check_hash, char* out_message, uint32_t capacity);

/* Host only, like aclhip_check_clip: what registration derives about the VALUES a (valid) clip can decode to, which decides the kernel
 * variants its instances run -- for tools ("do my clips take the short arithmetic?") and tests. Bits of *out_facts:
 *   ACLHIP_CLIP_FACT_SHORT_EXACT_MATH  no quantized rotation sample can hand the kernels a square root argument in (0, 2^-96) or a
 *                                      norm outside [2^-126, 2^126]: the short correctly rounded square root / reciprocal run
 *                                      (same bits, fewer instructions: DESIGN.md 4.1);
 *   ACLHIP_CLIP_FACT_RAW_ROTATIONS     some rotation sub-track is stored raw (fp32) in some segment;
 *   ACLHIP_CLIP_FACT_NEGATIVE_SCALE    some scale may decode to a negative component: the pose consumers compile rtm::qvv_mul's
 *                                      matrix route in while such a clip is registered.
 * Scalar track lists: 0. No reference counterpart (the reference has one code path). */
#define ACLHIP_CLIP_FACT_SHORT_EXACT_MATH 1u
#define ACLHIP_CLIP_FACT_RAW_ROTATIONS 2u
#define ACLHIP_CLIP_FACT_NEGATIVE_SCALE 4u
aclhip_status aclhip_analyze_clip(const void* compressed_tracks, uint64_t size, int check_hash, uint32_t* out_facts);

/* Replaces decompression_context::is_bound_to(const compressed_tracks&) (decompress.h:138): true when `clip`
 * was registered from a blob with the same hash and size. */
aclhip_status aclhip_clip_matches(const aclhip_context* context, aclhip_clip clip, const void* compressed_tracks, int* out_matches);

/* ---- databases (streamed keyframe tiers) ------------------------------------------------------- */

typedef struct aclhip_database_info
{
	uint32_t num_clips;
	uint32_t num_segments;
	uint32_t max_chunk_size;
	uint32_t num_chunks[2];					/* [0] medium importance tier, [1] low importance tier */
	uint32_t num_loaded_chunks[2];
	uint32_t bulk_data_size[2];
} aclhip_database_info;

/* Replaces database_context::initialize(allocator, database, medium_streamer, low_streamer)
 * (decompression/database/database.h:116; impl/database.impl.h): registers a compressed_database (HOST pointer, `size` bytes).
 * Bulk data of the two tiers is given separately (split_database_bulk_data) or may be null when it is inline in the database.
 * A bulk data pointer given separately must address compressed_database::get_bulk_data_size(tier) bytes (database_header::
 * bulk_data_size, aclhip_database_info::bulk_data_size after aclhip_check_database): like the reference's streamers, the call takes
 * no size for it and trusts the header the caller paired it with.
 * The bulk data is copied once into PINNED host memory -- the streamer's backing store -- and HBM buffers of the same size are
 * reserved; nothing is resident on the GPU until aclhip_database_stream_in. The runtime tier metadata the decoder reads
 * (database_runtime_segment_header::tier_metadata, core/impl/compressed_headers.h:404-422) lives in HBM. */
aclhip_status aclhip_register_database(aclhip_context* context, const void* compressed_database, uint64_t size,
	const void* bulk_data_medium, const void* bulk_data_low, int check_hash, aclhip_database* out_database);
aclhip_status aclhip_unregister_database(aclhip_context* context, aclhip_database database);

/* Replaces compressed_database::is_valid(check_hash) (core/impl/compressed_database.impl.h:142-163) as a host only call, with the
 * checks of aclhip_register_database (chunk and segment headers inside the bulk data, bulk data hashes). */
aclhip_status aclhip_check_database(const void* compressed_database, uint64_t size, const void* bulk_data_medium, const void* bulk_data_low,
	int check_hash, char* out_message, uint32_t capacity);
aclhip_status aclhip_get_database_info(const aclhip_context* context, aclhip_database database, aclhip_database_info* out_info);

/* Replaces decompression_context::initialize(const compressed_tracks&, const database_context&) (decompress.h:108;
 * impl/decompress.impl.h:85-113): like aclhip_register_clip for a clip that database.contains(). */
aclhip_status aclhip_register_clip_with_database(aclhip_context* context, const void* compressed_tracks, uint64_t size, int check_hash,
	aclhip_database database, aclhip_clip* out_clip);

/* Replace database_context::stream_in / stream_out(tier, num_chunks) (database/database.h:160-181, impl/database.impl.h:443-640):
 * tier 1 = medium importance, 2 = lowest importance. stream_in copies the next `num_chunks` missing chunks from pinned host
 * memory to HBM with hipMemcpyAsync on `stream` and then publishes their segments' tier metadata (stream ordered: decodes enqueued
 * later on the same stream see the new keyframes); stream_out retires the metadata of the first `num_chunks` resident chunks.
 * `out_num_chunks` (optional) receives how many chunks were actually moved (0 = done, like database_stream_request_result::done).
 * A request for 0 chunks follows the reference's arithmetic to the letter (database.impl.h:490-497,571-578: `first + 0 - 1` wraps
 * when the first candidate is chunk 0 and the WHOLE tier moves; with any other first candidate nothing does). */
aclhip_status aclhip_database_stream_in(aclhip_context* context, aclhip_database database, uint32_t tier, uint32_t num_chunks, void* stream, uint32_t* out_num_chunks);
aclhip_status aclhip_database_stream_out(aclhip_context* context, aclhip_database database, uint32_t tier, uint32_t num_chunks, void* stream, uint32_t* out_num_chunks);

/* Databases whose bulk data is served by the CALLER's streamers (acl::database_streamer objects, decompression/database/
 * database_streamer.h:95-175): only the compressed_database itself is known at registration. A stream-in request then hands over the
 * tier's bulk data as the streamer holds it (database_streamer::get_bulk_data(tier), HOST pointer; valid for the chunks the request
 * selects -- the same chunks the reference's database_context selects for the same request, database.impl.h:478-497): chunks seen for
 * the first time are validated and turned into tier metadata like aclhip_register_database does up front, their bytes are copied and
 * travel to HBM on `stream`. aclhip_database_stream_out and everything else work as for any database.
 * acl_gpu::database_context (acl_amd/csrc/acl_gpu_adapter.h) drives the caller's streamers through the reference's own
 * database_context and mirrors every completed request with these calls. */
aclhip_status aclhip_register_database_streamed(aclhip_context* context, const void* compressed_database, uint64_t size, int check_hash, aclhip_database* out_database);
aclhip_status aclhip_database_stream_in_from(aclhip_context* context, aclhip_database database, uint32_t tier, uint32_t num_chunks, const void* tier_bulk_data,
	void* stream, uint32_t* out_num_chunks);

/* Host only (no GPU work): strip_database_quality_tier (compression/compress.h:124, impl/compress.database.impl.h:1388-1525) --
 * the compressed_database without its medium (tier 1) or low (tier 2) importance tier, byte for byte what the reference builds
 * (it reserves room for the remaining tier's bulk data and sets its offset whether or not the bulk data is inline, and copies
 * only inline bulk data; so does this). The input must pass is_valid(true). Call with out_database NULL / capacity 0 for the
 * size. ACLHIP_ERROR_INVALID_ARGUMENT for the high importance tier (0) and for an empty tier, like the reference's errors. */
aclhip_status aclhip_strip_database_tier(const void* compressed_database, uint64_t size, uint32_t tier, void* out_database, uint64_t capacity, uint64_t* out_size);

/* ---- decompression ---------------------------------------------------------------------------- */

/* Replaces, for every instance i in [0, num_instances):
 *     context.seek(sample_times[i], rounding_policy);            (decompress.h:160; seek_v0 impl/decompression.transform.h:206-563)
 *     context.decompress_tracks(writer);                          (decompress.h:166; decompress_tracks_v0 :1526-1737)
 * with writer.write_rotation/translation/scale storing into
 *     (char*)poses + i * pose_stride_bytes + track_index * 48.
 * clips / sample_times / poses are DEVICE pointers; pose_stride_bytes must be a multiple of 16 and at least
 * 48 * num_tracks of the largest clip referenced. One wavefront decodes one window of 312 pose quads (104 tracks) of one instance.
 *
 * A launch is shaped by its BATCH: a row of pose_stride_bytes holds at most pose_stride_bytes / 48 tracks, so that -- or the largest
 * registered clip, whichever is smaller -- decides how many wavefronts an instance gets and how much LDS each of them; what else the
 * context holds (a 551-bone crowd leader next to the 100-bone characters of this batch) does not matter. The reference sizes its work
 * per clip (impl/decompression.transform.h:1526-1540). The kernels check every clip they meet against the launch and REFUSE -- count,
 * leave the pose row untouched: the reference's silent return, :1532-1537 -- an instance whose clip has more tracks than the stride
 * holds, more pose windows than the launch has wavefronts for or a window larger than the launch's LDS slots: a caller's stride that
 * is too small never writes outside its row, and a captured hipGraph replayed after a LARGER clip was registered refuses that
 * clip's instances (aclhip_get_rejected_instance_count) instead of decoding them into a launch shaped before the clip existed. Keep
 * rows as narrow as the batch needs: a stride of 14 400 bytes makes every instance a three-wavefront job. */
aclhip_status aclhip_decompress_tracks_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, void* poses, uint64_t pose_stride_bytes, void* stream);

/* Same, with the pose of instance i stored at row rows[i] of the pose buffer instead of row i (`rows`: DEVICE array of
 * num_instances distinct row indices): separates the order in which instances are decoded from where their poses go.
 * Scattered rows cost write locality: 256 clips decoded in aclhip_order_instances_for_locality order take 50 us with their
 * poses in decode order and 62 us scattered back to the original rows -- prefer numbering the rows in decode order. */
aclhip_status aclhip_decompress_tracks_batch_rows(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* rows,
	uint32_t num_instances, const aclhip_decompress_params* params, void* poses, uint64_t pose_stride_bytes, void* stream);

/* aclhip_decompress_tracks_batch with an output descriptor (NULL = QVV48, nothing skipped, row i): the pose of instance i starts at
 * (char*)poses + row * pose_stride_bytes and holds num_tracks records of 48 / 40 / 32 bytes in the chosen layout;
 * pose_stride_bytes must be a multiple of 16 and at least that size -- and should be a multiple of 64 (the HBM access granule): with
 * rows that start between granules every 1 KiB store of every other pose straddles them (QVV40, 100 bones: 4000 byte rows 82 us per
 * 64k poses, 4032 byte rows 44 us). Same values as the QVV48 decode, compared through the layout. */
aclhip_status aclhip_decompress_tracks_batch_out(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_output_desc* output, void* poses, uint64_t pose_stride_bytes, void* stream);

/* Bytes one track takes in a pose of `layout` (48 / 40 / 32); 0 for an unknown layout. */
uint32_t aclhip_layout_bytes_per_track(uint32_t layout);

/* ---- track maps: clips whose track order is not the skeleton's -------------------------------------
 * The run time form of the INDEX side of the track_writer protocol: track_writer::write_rotation / write_translation /
 * write_scale(track_index, value) (core/track_writer.h) hand the writer an index and the writer stores wherever it likes. An engine's
 * writer sends track t of a compressed clip -- which carries only the bones it animates, in its own order -- to the slot of its bone in
 * the SKELETON's pose; the bones the clip does not carry keep the reference pose. A registered map is that table; the mapped decode
 * below writes the pose in slot order in the ONE trip to HBM the decode makes anyway.
 *
 * aclhip_register_track_map: `track_to_slot` is a HOST array of `num_tracks` entries (the caller may free it when the call returns):
 * track_to_slot[t] is the record of the pose row track t is written to, in [0, num_slots), or ACLHIP_TRACK_DROPPED: the track is not
 * written at all. Refused with ACLHIP_ERROR_INVALID_ARGUMENT (the message names the first offending track): a slot >= num_slots, two
 * tracks mapped to one slot, num_tracks == 0, num_slots == 0, null pointers. The table and the sorted list of UNMAPPED slots (slots of
 * [0, num_slots) no track maps to; a dropped track maps to none) are uploaded on the context's own stream; only the calling thread
 * waits. Handles are small numbers >= 1; 0 is the null handle. The device's map table is allocated once, at the first registration
 * (ACLHIP_MAX_TRACK_MAPS records), and never moves: a captured hipGraph that names a map stays valid while other maps come and go.
 * Identical maps are not shared: every registration has a device image of its own (a few hundred bytes). */
typedef uint32_t aclhip_track_map;		/* handle returned by aclhip_register_track_map; 0 = none */
#define ACLHIP_TRACK_DROPPED 0xFFFFFFFFu
#define ACLHIP_MAX_TRACK_MAPS 16384u		/* live maps of one context, the null handle included */

typedef struct aclhip_track_map_info
{
	uint32_t num_tracks;
	uint32_t num_slots;
	uint32_t num_mapped;					/* tracks with a slot */
	uint32_t num_dropped;					/* tracks that are ACLHIP_TRACK_DROPPED */
	uint32_t num_unmapped_slots;			/* num_slots - num_mapped */
	uint32_t is_identity;					/* num_slots == num_tracks and track_to_slot[t] == t for every t */
	uint32_t is_order_preserving;			/* the slots of the mapped tracks ascend with the track index (the common case: contiguous runs stay contiguous) */
	uint32_t reserved;
} aclhip_track_map_info;

/* Host only (no context, no device): what registration checks and what aclhip_get_track_map_info reports. `message` (may be NULL,
 * `message_capacity` bytes) receives the reason when the map is refused; `out_info` may be NULL. */
aclhip_status aclhip_check_track_map(const uint32_t* track_to_slot, uint32_t num_tracks, uint32_t num_slots, aclhip_track_map_info* out_info,
	char* message, uint32_t message_capacity);

aclhip_status aclhip_register_track_map(aclhip_context* context, const uint32_t* track_to_slot, uint32_t num_tracks, uint32_t num_slots, aclhip_track_map* out_map);

/* Stream ordered retirement with the guarantees of aclhip_unregister_clip: launches ALREADY ENQUEUED on the streams this context
 * launched on still see the map (its record in the device table is cleared behind them, on a stream of the context's own); launches
 * that execute later refuse the handle (every instance that names it is counted, its row untouched); the map's memory and its handle
 * are recycled when both have happened. Nobody waits. */
aclhip_status aclhip_unregister_track_map(aclhip_context* context, aclhip_track_map map);

aclhip_status aclhip_get_track_map_info(const aclhip_context* context, aclhip_track_map map, aclhip_track_map_info* out_info);

typedef struct aclhip_track_mapping
{
	aclhip_track_map map;					/* used for every instance when instance_maps is NULL */
	const aclhip_track_map* instance_maps;	/* DEVICE [num_instances] or NULL: the map of instance i (the CALLER's instance index) */
	const void* fill_pose;					/* DEVICE or NULL: one pose of num_slots records in the launch's layout, 16 byte aligned, shared by the launch */
	uint32_t fill_unmapped;					/* 0: unmapped slots are left untouched; 1: written from fill_pose */
	uint32_t reserved;
} aclhip_track_mapping;

/* aclhip_decompress_tracks_batch_out with a destination index per track (track_writer::write_*(track_index, value),
 * core/track_writer.h). For instance i with clip c and map m: what the unmapped decode with the same `params` / `output` (may be
 * NULL) stores in record t of the row is stored in record m[t] instead -- same bits, same layout (QVV48 / QVV40 / QV32). Everything
 * `params` and `output` express keeps its meaning and stays indexed by TRACK: rounding and looping policies, default sub-track modes
 * (a skipped default leaves its bytes untouched AT THE MAPPED SLOT), skip_tracks / mask_table (one byte per track),
 * instance_track_counts (the first K tracks are decoded; their slots are their map's), rows.
 *   The row holds num_slots records. The launch is shaped like the unmapped one (min(largest registered clip, records the stride
 * holds) in pose windows of 104 tracks). The kernel refuses and counts (aclhip_get_rejected_instance_count; the row stays untouched)
 * an instance whose clip the unmapped decode would refuse -- in particular a clip with more tracks than the stride holds records,
 * whatever its map drops --, whose map handle is unknown or retired, whose map was made for another track count than its clip's, or whose
 * num_slots records do not fit pose_stride_bytes. No instance writes outside its row, whatever handle the device array holds.
 *   Unmapped slots (bones the clip does not animate): with fill_unmapped = 1 every slot of the instance's map that no track maps to is
 * written from fill_pose -- whole records, whatever `output` skips -- by the same launch (the list is split between the instance's
 * wavefronts), so the row leaves the kernel complete; tracks beyond an instance's track count are mapped, not filled. With
 * fill_unmapped = 0 those bytes are left untouched (the caller filled the buffer once; only animated slots change per frame).
 *   ACLHIP_ERROR_INVALID_ARGUMENT: mapping == NULL, a null map handle without instance_maps, fill_unmapped = 1 without a fill_pose,
 * a fill_pose that is not 16 byte aligned.
 *   What it costs (MI355X, 65 536 instances of the 100-bone clip, QVV48, tools/mapped_decode.py; DESIGN.md 4.8 has the table and the
 * counters): the unmapped decode takes 52 us; the identity map 77 us; a map into 128 slots 141 us without the fill and 95 us WITH it -- rows
 * written whole are cheaper than rows with holes, whose 64 byte granules are written in part. A RANDOM permutation into 128 slots costs what an
 * order-preserving one does (142 us): for QVV48 poses of one window with nothing skipped the row is gathered out of LDS in slot order, so the
 * permutation loses no write locality. Every other setting (poses of several windows, QVV40 / QV32, skips) stores scattered records, where a random
 * permutation measured 297 us on the same batch. Decode + one scatter pass, what a caller did before, takes 285 / 296 / 382 / 346 us for the
 * four cases: the mapped launch is 2.0 to 4.0 x faster than that, but it is not free.
 *   The pose consumers take maps through aclhip_decompress_poses_batch_mapped (skeletons, below). Still not mapped (the handle does not
 * preclude them): instance lists (aclhip_decompress_tracks_list), local space single track requests (the object space ones take maps:
 * aclhip_decompress_bone_object_batch_mapped), scalar track lists, the host convenience forms. ACLHIP_DECODE_FAST is accepted and changes nothing. */
aclhip_status aclhip_decompress_tracks_batch_mapped(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_output_desc* output, const aclhip_track_mapping* mapping, void* poses, uint64_t pose_stride_bytes, void* stream);

/* Host only (no GPU work): a decode order for a batch that draws on many clips -- a permutation of [0, num_instances) for the
 * instance list `clips` (HOST array) under which every clip is decoded on ONE XCD (workgroup b of a launch runs on XCD b % 8,
 * each XCD has its own L2; a clip that straddles the boundary between two XCDs' shares is decoded on both), next to its other
 * instances. Use: clips'[k] = clips[out_order[k]], sample_times'[k] = sample_times[out_order[k]], pose k of the launch belongs
 * to instance out_order[k]. 64k instances over 256 clips: 61 -> 50 us, the time of a single-clip batch; a batch of one clip is
 * unaffected. `context` tells how many wavefronts a pose of the largest registered clip takes (may be NULL: one).
 * Stable: instances of one clip keep their relative order. */
aclhip_status aclhip_order_instances_for_locality(const aclhip_context* context, const aclhip_clip* clips, uint32_t num_instances, uint32_t* out_order);

/* aclhip_order_instances_for_locality for a caller that knows the pose size instead of holding a context: windows_per_instance =
 * ceil(3 * num_tracks of the largest clip / ACLHIP_WINDOW_QUADS) wavefronts per pose (1 up to 104 tracks). Host only. */
aclhip_status aclhip_order_instances_for_pose_windows(uint32_t windows_per_instance, const aclhip_clip* clips, uint32_t num_instances, uint32_t* out_order);

/* Wavefronts per instance of the launch aclhip_decompress_tracks_batch[_out] makes for poses of `layout` in rows of `pose_stride_bytes`
 * with the clips registered now: min(largest registered clip, tracks the row holds) in pose windows of 104 tracks. Which slot of a
 * launch runs on which XCD follows from it: the value to order an instance list for (aclhip_order_instances_for_pose_windows,
 * aclhip_order_instances_device_for_windows). aclhip_order_instances_for_locality / _device assume rows as wide as the largest
 * registered clip. */
aclhip_status aclhip_pose_windows_of_launch(aclhip_context* context, uint32_t layout, uint64_t pose_stride_bytes, uint32_t* out_windows_per_instance);

/* The same order computed on the GPU for instance lists that live there (all pointers DEVICE pointers, stream ordered: ONE launch
 * on `stream` -- at most 64 workgroups that meet at barriers in global memory; three launches for registries of more than 8 192
 * clips --, scratch kept per stream by the context at a fixed size and address, no host synchronization). The one launch form needs all
 * its workgroups resident together: its grid is sized from the occupancy query to fit an idle device many times over. Should a barrier
 * not open within seconds all the same (dozens of such launches of other processes sharing the device), the launch GIVES UP without
 * placing anything -- no trap, the queue stays healthy --, the next ordering call on the stream returns ACLHIP_ERROR_DEVICE (once: the
 * order that launch was to write is invalid, order again) and the stream uses the three launch form from then on. Writes the permutation to out_order and,
 * when the pointers are not NULL, the permuted lists out_clips[k] = clips[out_order[k]], out_sample_times[k] =
 * sample_times[out_order[k]] (the arguments of the decode that follows on the same stream; rows = out_order puts the poses back
 * in the caller's rows). Which instance of a clip takes which of the clip's slots is decided by atomics: every call returns a valid
 * order, not the same one. The first call on a stream allocates that stream's scratch: make it before capturing the stream into a
 * hipGraph. A captured ordering HOLDS the scratch of the stream it was captured on: launch the graph on that stream (or at least never
 * while that stream, or another replay, orders -- two orderings that share a scratch at the same time write each other's counters; such
 * a launch places nothing out of bounds and raises the same failure as a barrier that does not open, but its order is not valid).
 * (PyTorch's CUDAGraph.replay() launches on the CURRENT stream, not on the capture stream: wrap it in `with torch.cuda.stream(s)`.)
 * An instance list usually outlives a frame (which character plays which clip changes rarely, the
 * sample times every frame): order once, keep the lists in that order. */
aclhip_status aclhip_order_instances_device(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	uint32_t* out_order, aclhip_clip* out_clips, float* out_sample_times, void* stream);
/* The same for launches of `windows_per_instance` wavefronts per pose (aclhip_pose_windows_of_launch) instead of the largest registered clip's. */
aclhip_status aclhip_order_instances_device_for_windows(aclhip_context* context, uint32_t windows_per_instance, const aclhip_clip* clips, const float* sample_times,
	uint32_t num_instances, uint32_t* out_order, aclhip_clip* out_clips, float* out_sample_times, void* stream);

/* ---- persistent instance lists: the library keeps the decode order -------------------------------------------------------------
 * (No reference counterpart: the reference decodes one pose per call. SURVEY.md section 7: "sort/bucket instances by clip for L2
 * locality".) A batch that draws on hundreds of clips decodes a fifth faster in locality order (aclhip_order_instances_for_locality),
 * but ordering a list costs more than one decode of it gains. Which character plays which clip changes rarely, the sample times
 * every frame: an instance list object keeps the clip assignment of `num_instances` instances IN DECODE ORDER across frames.
 *   aclhip_instance_list_set_clips   every instance's clip (device array in the caller's instance order); orders the list on `stream`
 *   aclhip_instance_list_update      instances[k] now plays clips[k] (device arrays, `count` entries, stream ordered). The instance keeps
 *                                    its slot; once an eighth of the list has changed since it was last ordered, the next decode
 *                                    re-orders it first (one launch, on the decode's stream)
 *   aclhip_decompress_tracks_list    decodes the list: sample_times[i] is instance i's sample time (the caller's order, gathered through
 *                                    the list's order by the decode itself). Poses land in SLOT order (pose row j = instance order[j],
 *                                    aclhip_instance_list_get_order) -- 1 KiB stores to consecutive rows, what the write path likes -- or,
 *                                    with poses_in_instance_order != 0, in row i for instance i (scattered rows: measured 20 % slower).
 *                                    `output` as in aclhip_decompress_tracks_batch_out (its `rows` must be NULL), or NULL.
 *   aclhip_instance_list_attach      instead of set_clips + update: the list decodes the CALLER's own clip array (device, `num_instances`
 *                                    entries in the caller's instance order, valid and in place for as long as the list is attached to
 *                                    it). The caller's animation graph writes clip changes straight into that array -- no update launch,
 *                                    no copy: a decode reads caller_clips[order[j]] for slot j (round 4 measured the library's own update
 *                                    launch at 5.3 us per frame for 655 changed instances; the extra dependent load this form costs a
 *                                    wavefront is hidden). An instance that changed clip is still decoded correctly, just no longer next
 *                                    to its clip's other instances;
 *   aclhip_instance_list_note_changes  tells an attached list that `count` of its instances changed clip since the last call (a host
 *                                    side number, nothing is read): once an eighth of the list has changed, the next decode re-orders it
 *                                    from the caller's array as it is then.
 * A list is ordered for the shape of the launches that decode it (wavefronts per pose: aclhip_pose_windows_of_launch); a decode whose pose
 * stride gives another shape than the list was last ordered for re-orders it first.
 * All calls of one list must be made in stream order (one stream, or the caller's events between streams). WHEN a list is re-ordered
 * is decided on the host at the time of the call: a decode captured into a hipGraph replays what was decided when it was captured
 * (capture aclhip_order_instances_device + aclhip_decompress_tracks_batch instead when the order has to follow the replays' data).
 * An update must not name an instance twice: the two entries race, and the clip that plays until the next re-order need not be the one
 * that plays after it (memory safe, but undefined which). Clip handles are not validated here: the decode refuses unknown ones (counted). */
typedef uint32_t aclhip_instance_list;

aclhip_status aclhip_instance_list_create(aclhip_context* context, uint32_t num_instances, aclhip_instance_list* out_list);
aclhip_status aclhip_instance_list_destroy(aclhip_context* context, aclhip_instance_list list);
aclhip_status aclhip_instance_list_set_clips(aclhip_context* context, aclhip_instance_list list, const aclhip_clip* clips, void* stream);
aclhip_status aclhip_instance_list_update(aclhip_context* context, aclhip_instance_list list, const uint32_t* instances, const aclhip_clip* clips, uint32_t count, void* stream);
aclhip_status aclhip_instance_list_attach(aclhip_context* context, aclhip_instance_list list, const aclhip_clip* caller_clips, void* stream);
aclhip_status aclhip_instance_list_note_changes(aclhip_context* context, aclhip_instance_list list, uint32_t count);
aclhip_status aclhip_decompress_tracks_list(aclhip_context* context, aclhip_instance_list list, const float* sample_times, const aclhip_decompress_params* params,
	const aclhip_output_desc* output, int poses_in_instance_order, void* poses, uint64_t pose_stride_bytes, void* stream);
/* the list's order, slot -> instance (device pointer, num_instances entries; contents change when the list is re-ordered, stream
 * ordered with the decodes) and how often the list has been (re-)ordered so far */
aclhip_status aclhip_instance_list_get_order(aclhip_context* context, aclhip_instance_list list, const uint32_t** out_order, uint64_t* out_num_orderings);

/* Host only (no GPU work): the order of a single track request list that draws on many clips -- a permutation of [0, num_requests)
 * for the request list `clips` (HOST array: the clip of every request) under which the requests are bucketed by clip (stable) and every
 * clip's requests run on ONE XCD (workgroup b of aclhip_decompress_track_batch takes requests 256 b .. 256 b + 255 and runs on XCD
 * b % 8; each XCD has its own L2). Use: clips'[k] = clips[out_order[k]], likewise sample times and track indices; transform k of the
 * launch belongs to request out_order[k]. For request lists that persist across frames (the same bones of the same characters, new
 * sample times): 4 M requests over 256 clips, 173 us as drawn, 77 us sorted by clip, 68 - 74 us in this order (HBM traffic 4.0 x the
 * algorithmic bytes as drawn, 0.98 x in this order). */
aclhip_status aclhip_order_track_requests_for_locality(const aclhip_clip* clips, uint32_t num_requests, uint32_t* out_order);

/* Replaces seek() + decompress_track(track_indices[i], writer) (decompress.h:172; decompress_track_v0 :1753-2050):
 * one 48 byte qvv per instance at (char*)transforms + i * 48. All pointers are DEVICE pointers.
 * Any order of requests is decoded; the ORDER decides what the launch fetches: 64 consecutive requests share a wavefront, and requests
 * of many clips are best bucketed by clip -- aclhip_order_track_requests_for_locality above gives the order (4 M requests over 256
 * clips: 173 us as drawn, 77 us sorted by clip = the time of one clip, 68 - 74 us in the library's order; profiles/r06_experiments.md 5b). */
aclhip_status aclhip_decompress_track_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* track_indices,
	uint32_t num_instances, const aclhip_decompress_params* params, void* transforms, void* stream);

/* The same order computed on the GPU for request lists built there every frame (IK targets, attachment bones, a crowd's root bones).
 * All pointers are DEVICE pointers; stream ordered on `stream`: three launches (count per clip, scan, scatter), no host
 * synchronization. Writes the permutation to out_order (required) and, when the pointers are not NULL, out_clips[k] =
 * clips[out_order[k]], out_sample_times[k] = sample_times[out_order[k]], out_track_indices[k] = track_indices[out_order[k]] (the
 * arguments of the aclhip_decompress_track_batch that follows on the same stream) and the inverse permutation
 * out_positions[out_order[k]] = k (request i's transform is transform out_positions[i] of that launch). The layout is
 * aclhip_order_track_requests_for_locality's: requests bucketed by clip in ascending handle order, every XCD one contiguous range
 * of that sequence. Which request of a clip takes which of the clip's slots is decided by atomics: every call returns a valid order,
 * not a stable or reproducible one -- but clips[out_order[k]] equals the host order's clips[host_order[k]] at every k whose handle
 * is registered. Handles past the registry share the last bucket, out-of-range track indices are ordered like any other request:
 * the decode refuses (and counts) both. Scratch and failure protocol are aclhip_order_instances_device's: the stream's ordering
 * scratch is shared by both kinds of ordering, the first call on a stream allocates it (make it before capturing the stream into a
 * hipGraph; no later call allocates unless the registry grows), a captured ordering holds the scratch of its stream (replay it on
 * that stream), and an ordering that did not complete -- of either kind -- makes the next ordering call on the stream return
 * ACLHIP_ERROR_DEVICE once. Measured for 4 M requests over 256 clips: the ordering 152 us as drawn at random (its
 * scatter writes every request's four words to scattered positions), 50 us for character-major lists (runs of one instance's
 * bones); ordering + decode 222 us against 176 us for the decode as drawn, 116 against 99 us character-major. So today it pays
 * where the ordered lists are decoded more than once, not for one decode of a list drawn at random. */
aclhip_status aclhip_order_track_requests_device(aclhip_context* context, const aclhip_clip* clips, const float* sample_times,
	const uint32_t* track_indices, uint32_t num_requests, uint32_t* out_order, aclhip_clip* out_clips, float* out_sample_times,
	uint32_t* out_track_indices, uint32_t* out_positions, void* stream);

/* aclhip_decompress_track_batch with the transform of request k stored at (char*)transforms + rows[k] * 48 instead of k * 48
 * (`rows`: DEVICE array of num_requests DISTINCT indices, not bounds checked, as in aclhip_decompress_tracks_batch_rows). With the
 * lists of aclhip_order_track_requests_device and rows = out_order the transforms of a device-ordered decode land in the
 * caller's request order. Refused requests and skipped default sub-tracks leave their row's bytes untouched, refusals are counted
 * (aclhip_get_rejected_instance_count). Every lane stores its own 48 bytes instead of a wave's three contiguous 1 KiB, and scattered
 * 48 byte records cost a lot of write bandwidth: 4 M requests over 256 clips take 640 us here against 76 us for the same ordered
 * decode in decode order, and order + this decode (793 us) is SLOWER than decoding the caller's list as drawn (176 us); 336 against
 * 68 us for character-major lists. Do not use it for throughput: decode in decode order and consume transform out_positions[i] for
 * request i. */
aclhip_status aclhip_decompress_track_batch_rows(aclhip_context* context, const aclhip_clip* clips, const float* sample_times,
	const uint32_t* track_indices, const uint32_t* rows, uint32_t num_requests, const aclhip_decompress_params* params,
	void* transforms, void* stream);

/* Convenience for host callers (the C++ mirror of decompression_context uses it with a batch of one): same as the two
 * calls above but every pointer is a HOST pointer; instance lists are uploaded, poses downloaded, the call is synchronous.
 * params->default_values / track_rounding_policies / instance_rounding_policies are HOST pointers here as well;
 * `default_values_count` is the number of qvv records default_values holds (1 for CONSTANT, num_tracks for VARIABLE). */
aclhip_status aclhip_decompress_tracks_host(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, uint32_t default_values_count, void* poses, uint64_t pose_stride_bytes);
aclhip_status aclhip_decompress_track_host(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* track_indices,
	uint32_t num_instances, const aclhip_decompress_params* params, uint32_t default_values_count, void* transforms);
/* aclhip_decompress_tracks_host with an output descriptor (output->rows, output->skip_tracks: HOST pointers or NULL; skip_tracks holds one
 * byte per track of the largest clip in the list). Skipped sub-tracks keep what `poses` held. */
aclhip_status aclhip_decompress_tracks_host_out(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, uint32_t default_values_count, const aclhip_output_desc* output, void* poses, uint64_t pose_stride_bytes);

/* ---- scalar track lists (float1f / float2f / float3f / float4f / vector4f) ------------------------
 * aclhip_register_clip accepts them like transform clips (decompression_context::initialize dispatches on the track type,
 * impl/decompress.impl.h:66-83 -> initialize_v0 impl/decompression.scalar.h:100-126; databases are not supported for them).
 *
 * Replace seek() + decompress_tracks(writer) for scalar track lists (seek_v0 / decompress_tracks_v0,
 * impl/decompression.scalar.h:182-480): instance i = (clips[i], sample_times[i]); track t of instance i is written as
 * num_components floats at (char*)values + i * stride_bytes + t * num_components * 4 -- what track_writer::write_float1 /
 * write_float2 / write_float3 / write_float4 / write_vector4 (core/track_writer.h:101-158) receive. Only the rounding / looping /
 * per track rounding members of `params` apply. Transform clips in the list are rejected (and counted), as scalar clips are by the
 * transform entry points. All pointers are DEVICE pointers; asynchronous on `stream`. */
aclhip_status aclhip_decompress_scalar_tracks_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, void* values, uint64_t stride_bytes, void* stream);

/* Replaces seek() + decompress_track(track_indices[i], writer) for scalar track lists (decompress_track_v0,
 * impl/decompression.scalar.h:482-715): num_components floats per instance at (char*)values + i * stride_bytes. */
aclhip_status aclhip_decompress_scalar_track_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* track_indices,
	uint32_t num_instances, const aclhip_decompress_params* params, void* values, uint64_t stride_bytes, void* stream);

/* The same with HOST pointers, synchronous (the C++ mirror of decompression_context uses them with a batch of one). */
aclhip_status aclhip_decompress_scalar_tracks_host(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, void* values, uint64_t stride_bytes);
aclhip_status aclhip_decompress_scalar_track_host(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* track_indices,
	uint32_t num_instances, const aclhip_decompress_params* params, void* values, uint64_t stride_bytes);

/* ---- every sample of a clip --------------------------------------------------------------------- */

/* The sampling loop of convert_track_list(allocator, compressed_tracks, track_array&) (compression/convert.h:52;
 * impl/convert.impl.h:150-260): for every sample i of the clip, seek(min(float(i) / sample_rate, duration), nearest) +
 * decompress_tracks, i.e. the clip's keyframes as the decoder sees them. Row i of `out` (DEVICE, `stride_bytes` apart) receives
 * what aclhip_decompress_tracks_batch / aclhip_decompress_scalar_tracks_batch write for one instance. `scratch` is a DEVICE
 * buffer of 8 * num_samples bytes (the generated instance list). `params` may be NULL; its rounding policy is ignored
 * (nearest, like the reference), the rest applies. Asynchronous on `stream`. */
aclhip_status aclhip_decompress_all_samples(aclhip_context* context, aclhip_clip clip, const aclhip_decompress_params* params,
	void* scratch, void* out, uint64_t stride_bytes, void* stream);

/* ---- pose consumers ---------------------------------------------------------------
 * What callers of decompress_tracks do next with the local space pose, fused into the decode so that the pose buffer makes
 * one trip to HBM instead of two or three: combining an additive clip with its base (acl::apply_additive_to_base,
 * core/additive_utils.h:150-160) and local -> object space (acl::local_to_object_space,
 * compression/transform_pose_utils.h:35-50). The reference writes both in Realtime Math; DESIGN.md 4.7 says what is restated
 * and how far an x86 build of the reference can be matched (rtm::quat_normalize starts from a hardware estimate). */

/* acl::additive_clip_format8 (core/additive_utils.h:43-68) */
typedef enum aclhip_additive_format
{
	ACLHIP_ADDITIVE_NONE = 0,		/* no base: the decoded pose passes through */
	ACLHIP_ADDITIVE_RELATIVE = 1,	/* qvv_mul(additive, base) */
	ACLHIP_ADDITIVE_ADDITIVE0 = 2,	/* transform_add0: scale = additive.scale * base.scale */
	ACLHIP_ADDITIVE_ADDITIVE1 = 3	/* transform_add1: scale = (1 + additive.scale) * base.scale */
} aclhip_additive_format;

#define ACLHIP_NO_PARENT 0xFFFFFFFFu

/* Parent of every transform of a registered transform clip (track_desc_transformf::parent_index, core/track_desc.h), copied.
 * parent_indices[i] < i for every transform but the roots (sorted parent first, as local_to_object_space assumes); transform 0
 * is a root whatever parent_indices[0] says (the reference never reads it), ACLHIP_NO_PARENT marks further roots.
 * num_tracks must be the clip's. Replaces a previous hierarchy of the clip (stream ordered like aclhip_unregister_clip: the old walk
 * schedule is recycled once the launches already enqueued have completed). */
aclhip_status aclhip_set_clip_hierarchy(aclhip_context* context, aclhip_clip clip, const uint32_t* parent_indices, uint32_t num_tracks);

/* The same with the parent indices the blob itself carries (compression_metadata_settings::include_parent_track_indices /
 * include_track_descriptions; compressed_tracks::get_parent_track_index, core/impl/compressed_tracks.impl.h:175-190): the caller passes
 * nothing. ACLHIP_ERROR_NO_METADATA when the clip was registered from a blob without them. */
aclhip_status aclhip_set_clip_hierarchy_from_metadata(aclhip_context* context, aclhip_clip clip);

/* Host only (no GPU work): how aclhip_set_clip_hierarchy schedules the object space walk of a hierarchy when up to
 * `transforms_per_step` transforms can be computed at once (64 / 32 / 16 / 8 for 1 / 2 / 4 / 8 instances per workgroup): every
 * transform is scheduled after its parent, at every step the ready transforms with the longest chain of descendants go first.
 * *out_num_steps: steps the walk takes; out_steps (optional, num_tracks entries): the 1-based step of each transform, 0 for roots.
 * ACLHIP_ERROR_INVALID_ARGUMENT when a transform precedes its parent. */
aclhip_status aclhip_plan_hierarchy_walk(const uint32_t* parent_indices, uint32_t num_tracks, uint32_t transforms_per_step, uint32_t* out_steps, uint32_t* out_num_steps);

typedef struct aclhip_pose_consumers
{
	uint32_t additive_format;			/* aclhip_additive_format: how each decoded instance combines with its base pose */
	uint32_t object_space;				/* 1: convert the (combined) local pose to object space with the clip's hierarchy */
	const aclhip_clip* base_clips;		/* DEVICE [num_instances] or NULL: the base of instance i is clip base_clips[i] sampled at ... */
	const float* base_sample_times;		/* DEVICE [num_instances] ... base_sample_times[i], decoded by the same wave (same params) */
	const void* base_poses;				/* DEVICE or NULL; used when base_clips is NULL: base pose i at base_poses + i * base_pose_stride_bytes, */
	uint64_t base_pose_stride_bytes;	/* 48 bytes per transform like the output; must not alias `poses` */
	/* Blend of K clip instances (no reference function -- the reference ships the arithmetic it is made of, quat_lerp's
	 * sign bias and normalize, math/quatf.h:170-211): instance i is the weighted combination of K = num_blend_clips clip instances,
	 * clips[i] at sample_times[i] first, then blend_clips[i * (K - 1) + j] at blend_sample_times[i * (K - 1) + j], j = 0 .. K - 2,
	 * with weights blend_weights[i * K + k]. All K clips of an instance must have the same number of tracks (else refused and
	 * counted). Per transform, in this operation order, fp32, never fused (ACLHIP_BLEND_* in DESIGN.md 4.7; oracle: aclo_blend_poses):
	 *     rotation     acc = q_0 * w_0;  for k = 1 .. K-1:  dot = ((acc.x q_k.x + acc.y q_k.y) + acc.z q_k.z) + acc.w q_k.w,
	 *                  acc = (q_k * (dot < 0 ? -w_k : w_k)) + acc;  rotation = quat_normalize(acc)   (the decoder's 1 / sqrt, math/quatf.h:200-211)
	 *     translation  acc = t_0 * w_0;  acc = (t_k * w_k) + acc         scale: like the translation
	 * The weights are the caller's (normally non negative with sum 1; they are not normalized here). The blended local pose then
	 * takes the place of the decoded one: additive apply and object space follow as configured above. */
	uint32_t num_blend_clips;			/* 0 or 1: no blend; 2 .. ACLHIP_MAX_BLEND_CLIPS */
	uint32_t flags;						/* ACLHIP_CONSUMERS_* */
	const aclhip_clip* blend_clips;		/* DEVICE [num_instances * (K - 1)] */
	const float* blend_sample_times;	/* DEVICE [num_instances * (K - 1)] */
	const float* blend_weights;			/* DEVICE [num_instances * K] */
} aclhip_pose_consumers;

#define ACLHIP_MAX_BLEND_CLIPS 4u

/* aclhip_pose_consumers::flags. By default the consumers' kernels follow the reference's x86 arithmetic one IEEE operation at a time
 * (core/additive_utils.h:128-160 and compression/transform_pose_utils.h:35-50 through rtm::quat_mul / qvv_mul, math/quatf.h:135-211 for
 * the decode) and are BIT EXACT with the oracle; much of a rotation's arithmetic is then correctly rounded square roots and divisions
 * (shorter exact forms of those run for clips whose registration proved them sufficient -- the bits do not change), and
 * these kernels keep the vector ALUs busy. ACLHIP_CONSUMERS_FAST is the opt-in for callers who
 * want the poses, not the bits: object space launches (object_space != 0, no blend) then compute the same formulas with the
 * hardware's 1 ulp square root / reciprocal square root, fused multiply-adds and quat_mul_vector3 as two cross products -- in the
 * decode of the instance and of its base, the fused additive apply and the walk. Rotations stay within 2e-6 of the default's per
 * component, translations within 2e-6 of the pose's extent (tests/test_gpu_consumers.py; DESIGN.md 4.7 has the measured figures).
 * Ignored (the default arithmetic runs) for local space output and for blends; mirrored transforms keep rtm's matrix route. A
 * workgroup whose local poses hold an infinity or a NaN (a clip that stores one) walks with the default arithmetic: the flag moves
 * numbers, never which words are NaNs (tests/test_gpu_nonfinite_samples.py). */
#define ACLHIP_CONSUMERS_FAST 1u

/* aclhip_decompress_tracks_batch followed by the consumers, in one kernel. `params` as for aclhip_decompress_tracks_batch but
 * restricted to what a consumer can work with -- the track_writer's own default sub-track modes, no per track rounding,
 * normalization != always -- else ACLHIP_ERROR_INVALID_ARGUMENT. Instances the kernel refuses (and counts, see
 * aclhip_get_rejected_instance_count) leave their pose untouched: unknown or scalar clips, object_space for a clip without
 * hierarchy, a base or blend clip with another number of tracks, a pose that does not fit its row. Poses are limited by the 160 KiB of
 * LDS a workgroup can use: about 3400 transforms (3100 with object space, 1700 when the base is a clip). Like every pose launch this one
 * is shaped by its batch -- pose_stride_bytes / 48 transforms, or the largest registered clip when that is smaller --
 * (ACLHIP_ERROR_INVALID_ARGUMENT when THAT does not fit): a 3 500-bone asset in the registry does not take the consumers away from the
 * 100-bone characters.
 * Asynchronous on `stream`. */
aclhip_status aclhip_decompress_poses_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, void* poses, uint64_t pose_stride_bytes, void* stream);

/* Same with host arrays (clips, times, base clips / times / poses, output): staged through temporary device buffers, synchronous. */
aclhip_status aclhip_decompress_poses_host(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, void* poses, uint64_t pose_stride_bytes);

/* ---- skeletons: the pose consumers in skeleton space ------------------------------------------------
 * A registered SKELETON is what the slot space of a set of track maps means: num_bones bones, their parents in slot order and a
 * reference (bind) pose of num_bones QVV48 records. With it the pose consumers work on clips that carry different tracks in different
 * orders: a walk cycle, an upper-body wave and a facial clip of one character are blended, layered additively and taken to object
 * space in ONE launch, each through its own track map, and the row leaves the kernel complete and in skeleton order.
 *
 * aclhip_register_skeleton: `parent_indices` (HOST, num_bones entries, or NULL) follows the rules of aclhip_set_clip_hierarchy --
 * parents first, bone 0 is a root, ACLHIP_NO_PARENT marks further roots -- and gets the same walk schedule (skeletons and clips with
 * identical hierarchies share one device image). A skeleton registered with NULL serves local space launches only. `reference_pose`
 * (HOST, num_bones x 48 bytes: rotation xyzw | translation xyz, pad | scale xyz, pad; the pads are stored as 0) must be finite.
 * Refused with ACLHIP_ERROR_INVALID_ARGUMENT before any device call (the message names the first offending bone): num_bones == 0 or
 * > 0xFFFF, a null reference pose, a bone ahead of its parent, a value that is not finite. Lifetime is a track map's: the device table
 * (ACLHIP_MAX_SKELETONS records) is allocated at the first registration and never moves, so a captured hipGraph that names a
 * skeleton stays valid while others come and go; handle 0 is null; uploads go on the context's own stream; unregistration is stream
 * ordered (launches already enqueued still see the skeleton, later ones refuse it) and nobody waits. */
typedef uint32_t aclhip_skeleton;		/* handle returned by aclhip_register_skeleton; 0 = none */
#define ACLHIP_MAX_SKELETONS 1024u		/* live skeletons of one context, the null handle included */

typedef struct aclhip_skeleton_info
{
	uint32_t num_bones;
	uint32_t has_hierarchy;				/* 0: registered without parent indices (local space only) */
	uint32_t num_roots;					/* 0 without hierarchy */
	uint32_t depth;						/* bones on the longest chain from a root to a leaf; 0 without hierarchy */
	uint32_t walk_steps;				/* steps of the object space walk at 16 transforms per step (aclhip_plan_hierarchy_walk); 0 without hierarchy */
	uint32_t has_negative_scale;		/* the reference pose holds a scale below zero (launches that multiply transforms then carry rtm::qvv_mul's matrix route) */
	uint32_t reserved[2];
} aclhip_skeleton_info;

/* Host only (no context, no device): what registration checks and what aclhip_get_skeleton_info reports. `message` (may be NULL,
 * `message_capacity` bytes) receives the reason when the skeleton is refused; `out_info` may be NULL. */
aclhip_status aclhip_check_skeleton(const uint32_t* parent_indices, const void* reference_pose, uint32_t num_bones,
	aclhip_skeleton_info* out_info, char* message, uint32_t message_capacity);

aclhip_status aclhip_register_skeleton(aclhip_context* context, const uint32_t* parent_indices, const void* reference_pose,
	uint32_t num_bones, aclhip_skeleton* out_skeleton);
aclhip_status aclhip_unregister_skeleton(aclhip_context* context, aclhip_skeleton skeleton);
aclhip_status aclhip_get_skeleton_info(const aclhip_context* context, aclhip_skeleton skeleton, aclhip_skeleton_info* out_info);

typedef struct aclhip_pose_mapping
{
	aclhip_skeleton skeleton;					/* for every instance when instance_skeletons is NULL */
	const aclhip_skeleton* instance_skeletons;	/* DEVICE [num_instances] or NULL */
	aclhip_track_map map;						/* the map of clips[i], for every instance when instance_maps is NULL */
	const aclhip_track_map* instance_maps;		/* DEVICE [num_instances] or NULL */
	const aclhip_track_map* blend_maps;			/* DEVICE [num_instances * (K - 1)], laid out like blend_clips; required when K > 1 */
	const aclhip_track_map* base_maps;			/* DEVICE [num_instances]; required when base_clips is set */
	uint32_t reserved[2];
} aclhip_pose_mapping;

/* aclhip_decompress_poses_batch in skeleton space. `params` and `consumers` keep their meaning and their restrictions. The output is
 * QVV48, B = num_bones records per row in skeleton order, EVERY slot written. The reference has no such function; the definition, from
 * pieces it does have -- take instance i with skeleton S (B bones, reference pose R, parents P):
 *   skeleton pose of a clip instance   skel(c, t, m, F)[s] = decode(c, t)[track] where m[track] == s, and F[s] for every slot no track
 *       maps to. Dropped tracks contribute nothing. decode is the unmapped decode under `params` with the instance's rounding and
 *       looping policies.
 *   the fill F   additive_format == NONE: F = R for every clip of the instance. Otherwise the instance's own clip and its blend partners
 *       are additive clips and a bone they do not animate must leave the base unchanged: their F is the ADDITIVE IDENTITY -- rotation
 *       (0, 0, 0, 1), translation 0, scale 1 for relative and additive0, scale 0 for additive1 (the reference compressor's default for
 *       additive clips) -- while a base clip always fills with R. A base pose BUFFER is in skeleton order already: B records,
 *       base_pose_stride_bytes >= 48 B.
 *   blend, additive apply, object space   today's operation orders (above; apply_additive_to_base; local_to_object_space) over the B
 *       skeleton poses, with P as the hierarchy. A filled slot takes the same arithmetic as a decoded one.
 * The clips of one instance may differ in track count: each only has to match its own map (map.num_tracks == clip.num_tracks), each
 * map the skeleton (map.num_slots == B). aclhip_set_clip_hierarchy plays no part: the hierarchy is the skeleton's.
 *   Refused and counted (aclhip_get_rejected_instance_count), the row untouched: an unknown or retired skeleton or map handle for any of
 * the instance's clips, either size mismatch, a scalar or unknown clip, object space on a skeleton without hierarchy, 48 B >
 * pose_stride_bytes or B beyond the launch's LDS image. No instance writes outside its row, whatever the device arrays hold.
 *   ACLHIP_ERROR_INVALID_ARGUMENT: mapping == NULL, no skeleton (a null handle without instance_skeletons), no map, K > 1 without
 * blend_maps, base_clips without base_maps, and everything aclhip_decompress_poses_batch refuses.
 *   The launch is shaped by its rows alone: pose_stride_bytes / 48 slots per LDS image, whatever clips are registered (a clip may have
 * more tracks than the skeleton has bones).
 *   Out of scope (nothing here precludes them): ACLHIP_CONSUMERS_FAST is accepted and the default arithmetic runs; the rotation |
 * translation images of unit-scale registries are not used; QVV40 / QV32 output; instance lists; the host convenience form; the C++
 * mirror in aclhip.hpp.
 *   What it costs: (MI355X, 65 536 instances of 100-bone clips, object space, tools/skeleton_poses.py; DESIGN.md 4.7 and
 * profiles/skeleton_poses.md have the table, the kernel traces and the counters): with identity maps the launch takes 1.21 - 1.27 x the
 * unmapped aclhip_decompress_poses_batch on the same batch (object space 106 vs 85 us, additive1 onto a base clip 181 vs 144 us, a blend of
 * three 233 vs 192 us), into 128 slots 1.46 - 1.60 x (137 / 281 us). It does NOT beat K launches of aclhip_decompress_tracks_batch_mapped
 * with fill -- the first step of what a caller does without it: 106 vs 77 us for K = 1 (0.73), 232 vs 232 us for K = 3 (1.00), 281 vs
 * 286 us for K = 3 into 128 slots (1.02). That floor holds none of the caller's further passes (the blend, the additive apply and the
 * walk each read and write the pose buffers again), which is what the launch is for. WRITE_SIZE / FETCH_SIZE equal the unmapped
 * launch's per byte of row: the difference is in-wave (dependent map loads in front of the gather and of every LDS write). */
aclhip_status aclhip_decompress_poses_batch_mapped(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping,
	void* poses, uint64_t pose_stride_bytes, void* stream);

/* ---- single bone requests in object space ------------------------------------------------------------
 * aclhip_decompress_track_batch returns a bone relative to its parent; a weapon socket, a camera on a head, a foot IK target or a hit
 * volume needs it in OBJECT space. These two launches return exactly that, without decoding and writing the whole pose: request k
 * writes one QVV48 record at (char*)transforms + k * 48. All pointers are DEVICE pointers; asynchronous on `stream`.
 *
 * aclhip_decompress_track_object_batch, by definition: transform k is record track_indices[k] of the row that
 * aclhip_decompress_poses_batch writes for (clips[k], sample_times[k]) under the same `params` with additive_format = NONE,
 * object_space = 1, no blend and default flags -- bit for bit. The operation order, with the clip's hierarchy from
 * aclhip_set_clip_hierarchy and the chain c_0 (a root) ... c_d = the bone:
 *     obj = local[c_0]                                   as decoded, nothing applied to it
 *     for j = 1 .. d:  obj = qvv_mul(local[c_j], obj)    child first, then parent; through rtm::qvv_mul's matrix route exactly where a
 *                                                        scale of either side is negative (aclhip_get_negative_scale_count's rule)
 *                      obj.rotation = quat_normalize(obj.rotation)
 * all in fp32, one IEEE operation at a time, never fused: what the object space walk does per (child, parent) pair. The seek runs once
 * per request; depth(bone) + 1 transforms are decoded, 48 bytes are written.
 *   `params` is restricted as for the pose consumers -- the track_writer's own default sub-track modes, no per track rounding,
 * normalization != always -- else ACLHIP_ERROR_INVALID_ARGUMENT. instance_rounding_policies and instance_looping_policies are indexed
 * by REQUEST, as in aclhip_decompress_track_batch. ACLHIP_DECODE_FAST and ACLHIP_CONSUMERS_FAST have no meaning here.
 *
 * aclhip_decompress_bone_object_batch_mapped, by definition: transform k is record bone_slots[k] of the row that
 * aclhip_decompress_poses_batch_mapped writes with additive_format = NONE, object_space = 1 and no blend. mapping->skeleton /
 * instance_skeletons and mapping->map / instance_maps are indexed by request; blend_maps and base_maps must be NULL. The chain runs
 * over skeleton slots with the skeleton's parents; local[s] = decode(c, t)[track] where the map sends `track` to slot s, or the
 * reference pose R[s] where no track maps to the slot. A skeleton whose R holds a negative scale takes the matrix route like a clip
 * that can decode one.
 *
 *   Refused and counted (aclhip_get_rejected_instance_count), the request's 48 bytes left untouched: an unknown or scalar clip; a clip
 * without a hierarchy (unmapped form) or a skeleton registered without one (mapped form); track_index >= num_tracks or bone_slot >=
 * num_bones; an unknown or retired skeleton or map handle; map.num_tracks != clip.num_tracks or map.num_slots != num_bones. No request
 * writes outside its own 48 bytes, whatever the device arrays hold. Nothing is uploaded at launch time: a captured hipGraph replays
 * while clips come and go (a clip or skeleton that may hand out a negative scale, registered behind the back of a launch captured
 * without the matrix route, is refused and counted, as the pose consumers do).
 *   The launches do NOT add to aclhip_get_negative_scale_count: requests share ancestors -- four sockets of one character walk the same
 * spine -- so a count of matrix products per launch would mean nothing.
 *   ACLHIP_ERROR_INVALID_ARGUMENT: null lists, transforms not 16 byte aligned, the params above; mapped form: mapping == NULL, no
 * skeleton (a null handle without instance_skeletons), no map, blend_maps or base_maps set.
 *   Out of scope (nothing here precludes them): blends, additive bases and masks per request; a _rows form; locality ordering of these
 * lists (aclhip_order_track_requests_for_locality / _device already order any (clip, time, index) list); the host convenience form; the
 * C++ mirror in aclhip.hpp.
 *   What it costs: MI355X, 65 536 characters of one 100-bone clip, character-major lists, against today's route (object space poses into
 * full rows, then a gather of the requested records; tools/socket_requests.py, profiles/socket_requests.md): one socket
 * per character 8.5 us shallow (depth 3) / 19.3 us deep (depth 11) against 99 us = 11.7 x / 5.1 x; four sockets 11.7 / 35.4 us against
 * 106 - 110 us = 9.3 x / 3.0 x; sixteen 43.5 / 120.3 us against 133 - 139 us = 3.2 x / 1.1 x. Over 256 clips as drawn the launch takes
 * about twice as long (1 socket 17.7 / 41.6 us, 4 sockets 20.9 / 59.6 us: 5.9 - 1.9 x). SIXTEEN DEEP SOCKETS PER CHARACTER DO NOT BEAT THE
 * WHOLE-POSE ROUTE: 1.11 x on one clip (inside the spread of the measurement) and 0.78 x over 256 clips (176 against 138 us) -- past
 * roughly a hundred chain transforms per character decode the pose and gather. Sockets that share ancestors decode them once each;
 * the per level decode is per lane, not packed across the wave (DESIGN.md 4.3 says what that leaves on the table). */
aclhip_status aclhip_decompress_track_object_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* track_indices,
	uint32_t num_requests, const aclhip_decompress_params* params, void* transforms, void* stream);
aclhip_status aclhip_decompress_bone_object_batch_mapped(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* bone_slots,
	uint32_t num_requests, const aclhip_decompress_params* params, const aclhip_pose_mapping* mapping, void* transforms, void* stream);

/* Host only (no context, no device, like aclhip_plan_hierarchy_walk): the chain the launches above walk for `bone`, root first, under
 * the rules of aclhip_set_clip_hierarchy -- transform 0 is a root whatever parent_indices[0] says, ACLHIP_NO_PARENT marks further
 * roots. *out_length: transforms on the chain, the bone included (depth + 1). out_chain (chain_capacity entries) may be NULL to query
 * the length only. ACLHIP_ERROR_INVALID_ARGUMENT when a transform of the hierarchy precedes its parent, bone >= num_tracks, or
 * chain_capacity is too small. */
aclhip_status aclhip_plan_bone_chain(const uint32_t* parent_indices, uint32_t num_tracks, uint32_t bone, uint32_t* out_chain, uint32_t chain_capacity, uint32_t* out_length);

/* ---- blend masks: a weight per bone for the blends of the skeleton space launch ---------------------
 * A blend of aclhip_pose_consumers has ONE weight per (instance, clip), applied to every bone: an upper-body clip layered over a walk
 * at 0.5 pulls the legs, which it does not animate and which hold the fill, half way to the reference pose. A registered BLEND MASK is
 * a table of B floats in skeleton slot order, each in [0, 1] ("layered blend per bone", an avatar mask), and
 * aclhip_decompress_poses_batch_masked is aclhip_decompress_poses_batch_mapped with an effective weight per (instance, clip, slot).
 *
 * aclhip_register_blend_mask: `weights` (HOST, num_slots floats). Refused with ACLHIP_ERROR_INVALID_ARGUMENT before any device call (the
 * message names the first offending slot): a null pointer, num_slots == 0 or > 0xFFFF, a value that is not finite or lies outside
 * [0, 1] (subnormals and -0 are inside). Lifetime is a track map's: the device table (ACLHIP_MAX_BLEND_MASKS records) is allocated at
 * the first registration and never moves, so a captured hipGraph that names a mask stays valid while others come and go; handle 0 is
 * null ("no mask": every slot 1); uploads go on the context's own stream; unregistration is stream ordered (launches already enqueued
 * still see the mask, later ones refuse it) and nobody waits. */
typedef uint32_t aclhip_blend_mask;			/* handle returned by aclhip_register_blend_mask; 0 = none: every slot 1 */
#define ACLHIP_MAX_BLEND_MASKS 4096u		/* live masks of one context, the null handle included */

typedef struct aclhip_blend_mask_info
{
	uint32_t num_slots;
	uint32_t num_zero;					/* slots whose weight is 0 (+0 or -0) */
	uint32_t num_one;					/* slots whose weight is 1 */
	uint32_t reserved;
} aclhip_blend_mask_info;

/* Host only (no context, no device): what registration checks and what aclhip_get_blend_mask_info reports. `message` (may be NULL,
 * `message_capacity` bytes) receives the reason when the mask is refused; `out_info` may be NULL. */
aclhip_status aclhip_check_blend_mask(const float* weights, uint32_t num_slots, aclhip_blend_mask_info* out_info, char* message, uint32_t message_capacity);

aclhip_status aclhip_register_blend_mask(aclhip_context* context, const float* weights, uint32_t num_slots, aclhip_blend_mask* out_mask);
aclhip_status aclhip_unregister_blend_mask(aclhip_context* context, aclhip_blend_mask mask);
aclhip_status aclhip_get_blend_mask_info(const aclhip_context* context, aclhip_blend_mask mask, aclhip_blend_mask_info* out_info);

#define ACLHIP_BLEND_WEIGHTED 0u		/* the masked weights are the blend's weights */
#define ACLHIP_BLEND_LAYERED 1u			/* the clips are layers, clip 0 at the bottom; the masked weight is a layer's opacity */

typedef struct aclhip_blend_masking
{
	uint32_t mode;								/* ACLHIP_BLEND_WEIGHTED / ACLHIP_BLEND_LAYERED */
	uint32_t reserved0;							/* 0 */
	const aclhip_blend_mask* instance_masks;	/* DEVICE [num_instances * K], laid out like blend_weights; entries may be 0 */
	uint64_t reserved[2];						/* 0 */
} aclhip_blend_masking;

/* aclhip_decompress_poses_batch_mapped with a weight per bone. Everything but the weight -- decode, fill, accumulation order, the final
 * quat_normalize, additive apply, object space walk, refusals -- is that launch's, unchanged. The definition, for instance i with
 * K = num_blend_clips clips, weights w_k = blend_weights[i * K + k], mask handles h_k = instance_masks[i * K + k] and slot s, all in fp32,
 * one IEEE operation at a time, never fused:
 *   1. e_k[s] = w_k when h_k == 0 (no mask), else e_k[s] = w_k * mask(h_k)[s].
 *   2. ACLHIP_BLEND_WEIGHTED: the weight of clip k at slot s is e_k[s].
 *      ACLHIP_BLEND_LAYERED: the clips are layers, k = 0 at the bottom, and e is a layer's opacity:
 *          r = 1; for j = K - 1 down to k + 1: r = r * (1 - e_j[s]);      e'_k[s] = e_k[s] * r
 *      and the weight of clip k at slot s is e'_k[s]. With e_0 == 1 these weights sum to 1 per bone, whatever the layers above do.
 *   3. Rotation, translation and scale of slot s follow the blend's operation order (aclhip_pose_consumers) with that weight in the
 *      place of w_k, quat_normalize at the end included. Nothing is renormalized, and nothing is skipped when a weight is 0 (x * 0 is
 *      added to the sum: it can turn a -0 into a +0, nothing else).
 * A slot whose weights are ALL 0 gets what the arithmetic gives -- the normalize of a zero quaternion, 0 / 0 --: the caller must avoid
 * it (keep clip 0's mask above 0 in weighted mode, e_0 == 1 in layered mode).
 *   With every handle 0, or with masks that are 1 everywhere, ACLHIP_BLEND_WEIGHTED gives the bits of aclhip_decompress_poses_batch_mapped.
 *   Refused and counted, the row untouched, on top of every refusal of the mapped launch: a mask handle that is unknown or retired, or
 * mask.num_slots != B, on any of the K entries of the instance.
 *   ACLHIP_ERROR_INVALID_ARGUMENT: masking == NULL, an unknown mode, reserved fields that are not 0, instance_masks == NULL,
 * num_blend_clips < 2, and everything aclhip_decompress_poses_batch_mapped refuses.
 *   Out of scope (nothing here precludes them): masks on the unmapped aclhip_decompress_poses_batch; the host convenience form, the
 * C++ mirror in aclhip.hpp and instance lists. (An additive layer's strength per bone: aclhip_additive_layering, below.)
 *   What it costs: DESIGN.md 4.7 ("Blend masks") and profiles/blend_masks.md (tools/blend_masks.py). */
aclhip_status aclhip_decompress_poses_batch_masked(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping, const aclhip_blend_masking* masking,
	void* poses, uint64_t pose_stride_bytes, void* stream);

/* ---- additive strength: an additive layer per instance and per bone --------------------------------
 * apply_additive_to_base takes the additive clip at full strength on every bone, as the reference function does. At run time a lean, a
 * breathing cycle, a recoil or an aim offset is faded in and out per character (a scalar in [0, 1]) and confined to part of the body (a
 * registered blend mask, above). aclhip_decompress_poses_batch_additive_weighted is aclhip_decompress_poses_batch_mapped with a strength
 * per (instance, slot) on the additive pose: decode, fill, the blend of K additive clips, the apply, the walk and the refusals are that
 * launch's, unchanged. (ABI version 6 still: an added struct and an added function, no existing struct changed.) */
typedef struct aclhip_additive_layering
{
	const float* instance_weights;				/* DEVICE [num_instances] or NULL: every instance 1 */
	const aclhip_blend_mask* instance_masks;	/* DEVICE [num_instances] or NULL; entries may be 0 (no mask: every slot 1) */
	uint64_t reserved[2];						/* 0 */
} aclhip_additive_layering;

/* The definition, for instance i and slot s, all in fp32, one IEEE operation at a time, never fused:
 *   1. w = instance_weights[i] (1 without the array).
 *   2. e[s] = w when the instance's mask handle h = instance_masks[i] is 0 (or there is no array), else e[s] = w * mask(h)[s].
 *   3. A[s] is the additive local transform of the slot as aclhip_decompress_poses_batch_mapped has it in front of
 *      apply_additive_to_base: the decoded or filled additive clip, or the normalized blend of the K additive clips.
 *   4. e[s] == 1.0f: A'[s] = A[s], bit for bit (the blend formula below renormalizes, which would change the bits of a rotation that is
 *      normalized already). So weights that are all 1 with null masks, or with masks that are 1 everywhere, give the bits of
 *      aclhip_decompress_poses_batch_mapped.
 *   5. Otherwise A'[s] is the two clip blend of aclhip_pose_consumers over (I, A[s]) with weights (u, e[s]), u = 1 - e[s], where I is the
 *      additive identity the mapped launch fills with: rotation (0, 0, 0, 1), translation 0, scale 1 (0 for ACLHIP_ADDITIVE_ADDITIVE1).
 *          rotation: acc = I.r * u; dot = ((acc.x q.x + acc.y q.y) + acc.z q.z) + acc.w q.w; acc = (q * (dot < 0 ? -e : e)) + acc; quat_normalize(acc)
 *          translation and scale: acc = I.t * u; acc = (t * e) + acc
 *      Weights are used as given, nothing is clamped. For e in [0, 1) the accumulated w lane is u + e |q.w| > 0: the normalize never
 *      sees a zero quaternion. Outside [0, 1] the arithmetic gives what it gives.
 *   6. The row is apply_additive_to_base(additive_format, base[s], A'[s]), then object space as configured.
 * e[s] == 0 applies the identity: the slot holds the base (through the apply's own arithmetic).
 *   Refused and counted, the row untouched, on top of every refusal of the mapped launch: a mask handle that is unknown or retired, or
 * mask.num_slots != B.
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message: layering == NULL, both arrays NULL (that is the
 * mapped launch), reserved fields that are not 0, additive_format == ACLHIP_ADDITIVE_NONE, and everything
 * aclhip_decompress_poses_batch_mapped refuses.
 *   Out of scope (nothing here precludes them): the unmapped aclhip_decompress_poses_batch; combining with aclhip_blend_masking; the
 * bounds entry point; several additive layers; the host convenience form; the C++ mirror in aclhip.hpp; instance lists.
 *   What it costs: NOT MEASURED YET (tools/additive_strength.py, profiles/additive_strength.md; DESIGN.md 4.7 "Additive strength"). */
aclhip_status aclhip_decompress_poses_batch_additive_weighted(aclhip_context* context, const aclhip_clip* clips, const float* sample_times,
	uint32_t num_instances, const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping,
	const aclhip_additive_layering* layering, void* poses, uint64_t pose_stride_bytes, void* stream);

/* ---- character bounds: one box per instance from the object space pose consumers -------------------
 * What a crowd does with an object space pose before it renders: one axis aligned box per character, for frustum, occlusion and LOD
 * culling. Without this launch a caller allocates the full row buffer (315 MB for 65 536 x 100 bones), runs the object space launch and
 * reads all of it back in a reduction pass of its own for 32 bytes per character. The object space launch has every pose complete in LDS
 * and one wave walks it from there to HBM: the box is a minimum / maximum over the translation quads that wave reads anyway.
 * (ABI version 6 still: an added struct and an added function, no existing struct changed.) */
typedef struct aclhip_pose_bounds
{
	void* bounds;					/* DEVICE, num_instances x 32 bytes, 16 byte aligned: min.x min.y min.z 0 | max.x max.y max.z 0 */
	const uint8_t* bone_flags;		/* DEVICE or NULL: one byte per transform of a row (pose_stride_bytes / 48 entries), launch wide like
									   aclhip_output_desc::skip_tracks; non-zero = the bone counts. NULL: every bone counts */
	uint64_t reserved[2];			/* 0 */
} aclhip_pose_bounds;

/* Which launch it is: aclhip_decompress_poses_batch when `mapping` is NULL, aclhip_decompress_poses_batch_mapped when `mapping` is set,
 * aclhip_decompress_poses_batch_masked when `masking` is set too. It takes the same `params` and `consumers`, refuses the same cases and
 * uses the same arithmetic; consumers->object_space must be set.
 *   The bounds of instance i: bounds[i].min / .max are the component-wise minimum / maximum, over the counted bones b, of
 * row_i[b].translation, where row_i is the row that launch writes for instance i. Comparison is as float values: a NaN coordinate is
 * ignored, the sign of a zero result is unspecified, the two pad lanes are 0. An instance with no counted bone -- an all-zero bone_flags,
 * a clip of zero tracks -- gets the EMPTY box: min = +inf, max = -inf. (min and max are exact and order independent: the box is that of
 * the row, bit for bit, whatever order the kernel takes the bones in.)
 *   poses != NULL: the rows are written as well, bit for bit what the launch without bounds writes. poses == NULL: no row is written --
 * the culling pass, 2 MB out for 65 536 characters. pose_stride_bytes keeps its meaning as the launch's shape in both cases:
 * pose_stride_bytes / 48 is the largest pose accepted, sizes the LDS image and gives the length of bone_flags; an instance whose pose
 * does not fit that shape is refused, as by the launch without bounds.
 *   A refused instance is counted in aclhip_get_rejected_instance_count exactly when the launch without bounds refuses it; its 32 bytes and
 * its row stay untouched. ACLHIP_CONSUMERS_FAST keeps its meaning where the underlying launch honours it (the unmapped one): the bounds are
 * then the minimum / maximum of the FAST rows. aclhip_get_negative_scale_count moves as it does for the launch without bounds.
 *   ACLHIP_ERROR_INVALID_ARGUMENT: bounds == NULL, bounds->bounds NULL or not 16 byte aligned, reserved fields that are not 0,
 * consumers->object_space == 0 (a local space translation is not a position), masking without mapping, and everything the underlying
 * launch refuses (poses may be NULL; when set it is 16 byte aligned like the stride). Decided before any device call, each with a message.
 *   Out of scope (nothing here precludes them): per-bone radii or padding of the box; the host convenience form; the C++ mirror in
 * aclhip.hpp; instance lists; bounds for the single-bone launches (aclhip_decompress_track_object_batch and its mapped form).
 *   What it costs: NOT MEASURED YET (tools/pose_bounds.py, profiles/pose_bounds.md). */
aclhip_status aclhip_decompress_poses_batch_bounds(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping /* NULL: unmapped */,
	const aclhip_blend_masking* masking /* NULL, or with mapping + blend */, const aclhip_pose_bounds* bounds, void* poses /* may be NULL */,
	uint64_t pose_stride_bytes, void* stream);

/* ---- pose buffers: object space and additive apply over a caller's poses ---------------------------
 * Every consumer above is fused into a decode. A caller who changes the local pose between the decode and the walk -- IK, look-at, ragdoll
 * or physics blending, procedural secondary motion, retargeting, or a pose it produced itself -- decodes with
 * aclhip_decompress_tracks_batch(_mapped) and hands the rows to aclhip_transform_poses_batch: the reference's free functions over pose
 * arrays, acl::local_to_object_space (compression/transform_pose_utils.h:42-56: "it is safe for both pose buffers to alias") and
 * acl::apply_additive_to_base (core/additive_utils.h:150-160), with the walk schedule, rtm::qvv_mul's matrix route and the normalize of
 * the fused launches. (ABI version 6 still: an added struct and an added function, no existing struct changed.) */
typedef struct aclhip_pose_buffer_consumers
{
	aclhip_skeleton skeleton;					/* for every instance when instance_skeletons is NULL */
	const aclhip_skeleton* instance_skeletons;	/* DEVICE [num_instances] or NULL */
	uint32_t object_space;						/* 1: local_to_object_space with the skeleton's parents */
	uint32_t additive_format;					/* aclhip_additive_format; NONE: no additive buffer */
	const void* additive_poses;					/* DEVICE or NULL: additive pose i at additive_poses + i * additive_pose_stride_bytes, QVV48, skeleton order */
	uint64_t additive_pose_stride_bytes;
	const aclhip_pose_bounds* bounds;			/* NULL, or one box per instance as aclhip_decompress_poses_batch_bounds defines it (object_space only) */
	uint64_t reserved[2];						/* 0 */
} aclhip_pose_buffer_consumers;

/* The definition. Instance i has skeleton S (consumers->skeleton, or instance_skeletons[i]) with B bones and parents P.
 *   1. L is the B QVV48 records at local_poses + i * local_pose_stride_bytes.
 *   2. With an additive format, A is the B records of the additive row and L'[b] = apply_additive_to_base(format, base = L[b],
 *      additive = A[b]) per bone: the operation the base_poses path of aclhip_decompress_poses_batch performs, with the roles of the two
 *      buffers as named here (the caller's local pose is the base, the additive buffer is what a decode would have produced). Without
 *      one, L' = L.
 *   3. With object_space, row i is local_to_object_space(P, L'): roots are copied as they are; every other bone is
 *      qvv_mul(child, object[parent]) -- rtm::qvv_mul's matrix route where a scale of either side is negative
 *      (aclhip_get_negative_scale_count's rule, and that counter moves as it does for a launch with a base pose buffer) -- then
 *      quat_normalize, the decoder's 1 / sqrt. Otherwise row i is L'.
 *   The arithmetic is the correctly rounded one of the fused launches, bit for bit the oracle's; nothing is assumed about a caller's
 * rotations or scales. The pads (the fourth float of a translation and of a scale): every transform that went through
 * apply_additive_to_base or through the walk's qvv_mul is written with both pads 0, whatever the inputs held. What went through neither --
 * a ROOT of an object_space launch without an additive buffer -- is copied whole, pads included: it keeps the bytes of L.
 *   All B records are written; bytes of a row behind B * 48 are untouched.
 *   In place: poses == local_poses with equal strides is allowed, and is the expected use -- a row is complete in LDS before any of it is
 * stored, and no wave reads another instance's row. Any other overlap of the output range with the input range, and any overlap with the
 * additive range, is ACLHIP_ERROR_INVALID_ARGUMENT; the host decides this from the three (pointer, stride, num_instances) ranges,
 * [pointer, pointer + stride * num_instances).
 *   Bounds (consumers->bounds): the same boxes, the same bone_flags, the same empty box and the same NaN rule as
 * aclhip_decompress_poses_batch_bounds, over the rows this launch writes; poses == NULL gives the boxes alone.
 *   Refused and counted (aclhip_get_rejected_instance_count), the row and the box untouched: an unknown or retired skeleton handle (0
 * included); object_space on a skeleton without hierarchy; B * 48 larger than any of the strides in use (local_pose_stride_bytes,
 * pose_stride_bytes when poses is set, additive_pose_stride_bytes with an additive format); B beyond the launch's LDS image. No instance
 * reads or writes outside its rows, whatever instance_skeletons holds. A skeleton unregistered after the launch was enqueued is still served.
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): consumers == NULL or
 * local_poses == NULL; no skeleton at all (skeleton == 0 and instance_skeletons == NULL); object_space == 0 with
 * ACLHIP_ADDITIVE_NONE (nothing to do); a format other than NONE without additive_poses, or the reverse; bounds without object_space;
 * poses == NULL without bounds; pointers or strides that are not 16 byte aligned; reserved fields that are not 0; a bounds struct
 * aclhip_decompress_poses_batch_bounds would refuse; a shape that does not fit 160 KiB of LDS; the overlaps above.
 *   The launch's shape comes from the rows alone, as for the mapped launch: pose_stride_bytes / 48 slots per LDS image (and entries of
 * bone_flags), or local_pose_stride_bytes / 48 when poses is NULL. Registered clips play no part. The launch goes on `stream`, can be
 * captured into a graph, and uploads nothing.
 *   Out of scope (nothing here precludes them): additive strength on buffers; QVV40 / QV32 rows; ACLHIP_CONSUMERS_FAST; the host
 * convenience form; the C++ mirror in aclhip.hpp; instance lists. (A blend of several buffers, with blend masks:
 * aclhip_blend_poses_batch, below. The way back, object_to_local_space and make-additive: aclhip_inverse_transform_poses_batch, below.)
 *   What it costs: NOT MEASURED YET (tools/pose_buffers.py, profiles/pose_buffers.md; DESIGN.md 4.7 "Pose buffers"). */
aclhip_status aclhip_transform_poses_batch(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes,
	uint32_t num_instances, const aclhip_pose_buffer_consumers* consumers, void* poses /* may be NULL with bounds */,
	uint64_t pose_stride_bytes, void* stream);

/* ---- blended pose buffers: the masked blend over a caller's poses ----------------------------------
 * The fused blend (aclhip_pose_consumers::num_blend_clips) and the fused masks (aclhip_decompress_poses_batch_masked) blend CLIPS. A
 * ragdoll or physics pose blended with the animated one per bone (hips 0, arms 1), an IK corrected pose cross-faded back to the decoded
 * one, a pose cached from a state machine's previous state blended with the pose just decoded: each has an operand that is no clip.
 * aclhip_blend_poses_batch is that blend -- the same weights, the same masks, the same two modes, the same arithmetic -- over K rows the
 * caller owns, with the object space walk and the boxes of aclhip_transform_poses_batch behind it in the same launch.
 * (ABI version 6 still: an added struct and an added function, no existing struct changed.) */
typedef struct aclhip_pose_buffer_blend
{
	aclhip_skeleton skeleton;					/* for every instance when instance_skeletons is NULL */
	const aclhip_skeleton* instance_skeletons;	/* DEVICE [num_instances] or NULL */
	uint32_t num_buffers;						/* K: 2 .. ACLHIP_MAX_BLEND_CLIPS */
	uint32_t mode;								/* ACLHIP_BLEND_WEIGHTED / ACLHIP_BLEND_LAYERED */
	const void* buffers[ACLHIP_MAX_BLEND_CLIPS];	/* DEVICE: pose i of buffer k at buffers[k] + i * buffer_stride_bytes[k], QVV48, skeleton order; entries >= K are NULL */
	uint64_t buffer_stride_bytes[ACLHIP_MAX_BLEND_CLIPS];
	const float* weights;						/* DEVICE [num_instances * K], laid out like blend_weights */
	const aclhip_blend_mask* instance_masks;	/* DEVICE [num_instances * K] or NULL (no masks); entries may be 0 */
	uint32_t object_space;						/* 1: local_to_object_space with the skeleton's parents behind the blend */
	uint32_t reserved0;							/* 0 */
	const aclhip_pose_bounds* bounds;			/* NULL, or boxes as aclhip_decompress_poses_batch_bounds defines them (object_space only) */
	uint64_t reserved[2];						/* 0 */
} aclhip_pose_buffer_blend;

/* The definition. Instance i has skeleton S (blend->skeleton, or instance_skeletons[i]) with B bones and parents P; X_k is the B QVV48
 * records at buffers[k] + i * buffer_stride_bytes[k].
 *   1. The effective weight of buffer k at slot s is that of steps 1 and 2 of aclhip_blend_masking's definition, with
 *      w_k = weights[i * K + k] and h_k = instance_masks[i * K + k] (0 when the array is NULL): e_k[s] in ACLHIP_BLEND_WEIGHTED,
 *      e'_k[s] in ACLHIP_BLEND_LAYERED -- buffer 0 at the bottom, the product of (1 - e_j) taken from the top layer down. Layered mode
 *      without masks is allowed: the opacity is then uniform per instance.
 *   2. Rotation, translation and scale of slot s follow the blend's operation order (aclhip_pose_consumers) with that weight:
 *      acc = X_0 * w, then for k = 1 .. K - 1 the sign biased accumulate against the running sum, quat_normalize at the end; fp32, one
 *      IEEE operation at a time, never fused. Nothing is renormalized and nothing is skipped when a weight is 0; a slot whose weights are
 *      ALL 0 gets what the arithmetic gives (0 / 0): the caller must avoid it, as under aclhip_blend_masking.
 *   3. With object_space, row i is local_to_object_space(P, blended), exactly as step 3 of aclhip_transform_poses_batch defines it: roots
 *      are copied, every other bone is qvv_mul(child, object[parent]) -- rtm::qvv_mul's matrix route where a scale of either side is
 *      negative, and aclhip_get_negative_scale_count moves as it does for that launch -- then quat_normalize, the decoder's 1 / sqrt.
 *      Otherwise row i is the blended local pose.
 *   4. Every record written has both pads 0 (the blend writes them so, roots included), whatever the inputs held. All B records are
 *      written; bytes of a row behind B * 48 are untouched.
 *   In place: poses may be exactly ONE of the inputs (the pointer and the stride of some buffers[k]) -- the expected use, blending into
 *   the animated buffer -- or disjoint from every input range. Any other overlap of the output range with an input range is
 * ACLHIP_ERROR_INVALID_ARGUMENT; the host decides this from the (pointer, stride, num_instances) ranges,
 * [pointer, pointer + stride * num_instances). The inputs are only read and may overlap each other freely. bounds->bounds
 * (num_instances x 32 bytes) must not overlap an input or the output.
 *   Bounds (blend->bounds): the same boxes, the same bone_flags, the same empty box and the same NaN rule as
 * aclhip_decompress_poses_batch_bounds, over the rows this launch writes; poses == NULL gives the boxes alone.
 *   Refused and counted (aclhip_get_rejected_instance_count), the row and the box untouched: an unknown or retired skeleton handle (0
 * included); object_space on a skeleton without hierarchy; B * 48 larger than any of the strides in use (each of the K
 * buffer_stride_bytes, pose_stride_bytes when poses is set); B beyond the launch's LDS image; on any of the K entries of the instance a
 * mask handle that is unknown or retired, or mask.num_slots != B. The refusal comes in front of any load of a row: no instance reads or
 * writes outside its own rows, whatever the device arrays hold. A skeleton or a mask unregistered after the launch was enqueued is still
 * served.
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): blend == NULL; K
 * outside 2 .. ACLHIP_MAX_BLEND_CLIPS; an unknown mode; a NULL entry among the first K buffers or a non-NULL entry behind them;
 * weights == NULL; no skeleton at all (skeleton == 0 and instance_skeletons == NULL); bounds without object_space; poses == NULL
 * without bounds; a pointer or a stride that is not 16 byte aligned; reserved fields that are not 0; a bounds struct
 * aclhip_decompress_poses_batch_bounds would refuse; a shape that does not fit 160 KiB of LDS; the overlaps above.
 *   The launch's shape comes from the rows alone: pose_stride_bytes / 48 slots per LDS image (and entries of bone_flags), or
 * buffer_stride_bytes[0] / 48 when poses is NULL. Registered clips play no part. The launch goes on `stream`, can be captured into a
 * graph, and uploads nothing.
 *   Out of scope (nothing here precludes them): an additive buffer or an additive strength in the same launch (chain
 * aclhip_transform_poses_batch on the blended rows); QVV40 / QV32 rows; ACLHIP_CONSUMERS_FAST; the host convenience form; the C++ mirror
 * in aclhip.hpp; instance lists.
 *   What it costs (one MI355X, 65 536 x 100 bones, medians of three runs): K = 2 162 us local / 177 us object space, K = 4 279 / 283 us,
 * with or without masks, against 110 us for aclhip_transform_poses_batch with object space on one of the same buffers, measured in the
 * same rounds: 1.5 x and 2.5 x its time for 1.5 x and 2.5 x its bytes, 0.67 - 0.73 of the HBM peak (tools/pose_buffer_blend.py,
 * profiles/pose_buffer_blend.md; DESIGN.md 4.7 "Blended pose buffers"). */
aclhip_status aclhip_blend_poses_batch(aclhip_context* context, const aclhip_pose_buffer_blend* blend, uint32_t num_instances,
	void* poses /* may be NULL with bounds */, uint64_t pose_stride_bytes, void* stream);

/* ---- inverse pose buffers: object -> local space and make-additive over a caller's poses ----------
 * aclhip_transform_poses_batch takes a pose into object space in one launch. Whatever is solved there -- foot IK, look-at, a ragdoll or
 * physics pose, an attachment constraint -- has to come back to local space before it can be blended, layered or cached, and an engine's
 * "make dynamic additive" node needs the difference of two poses. aclhip_inverse_transform_poses_batch is the inverse of the two steps of
 * aclhip_transform_poses_batch, in the opposite order: object -> local space with the skeleton's parents, then
 * acl::convert_to_relative / convert_to_additive0 / convert_to_additive1 (core/additive_utils.h:176-195) against a base pose buffer.
 * (ABI version 6 still: an added struct and an added function, no existing struct changed.) */
typedef struct aclhip_pose_buffer_inverse
{
	aclhip_skeleton skeleton;					/* for every instance when instance_skeletons is NULL */
	const aclhip_skeleton* instance_skeletons;	/* DEVICE [num_instances] or NULL */
	uint32_t local_space;						/* 1: object -> local with the skeleton's parents */
	uint32_t additive_format;					/* aclhip_additive_format; NONE: no base buffer */
	const void* base_poses;						/* DEVICE or NULL: base pose i at base_poses + i * base_pose_stride_bytes, QVV48, skeleton order, LOCAL space */
	uint64_t base_pose_stride_bytes;
	uint64_t reserved[3];						/* 0 */
} aclhip_pose_buffer_inverse;					/* 64 bytes, offsets 0 8 16 20 24 32 40 */

/* The definition. Instance i has skeleton S (inverse->skeleton, or instance_skeletons[i]) with B bones and parents P; X is the B QVV48
 * records at source_poses + i * source_pose_stride_bytes.
 *   1. With local_space: a root (a bone whose parent is ACLHIP_NO_PARENT; bone 0 is one) gives L[b] = X[b]; every other bone gives
 *      L[b] = qvv_mul(X[b], qvv_inverse(X[P[b]])) with its rotation through quat_normalize. qvv_inverse is rtm::qvv_inverse, in this
 *      order: the rotation conjugated (sign flips); scale^-1 = 1 / scale, the correctly rounded division; translation^-1 =
 *      -quat_mul_vector3(scale^-1 * translation, rotation^-1). qvv_mul is the walk's (lhs first), with rtm::qvv_mul's matrix route where
 *      a scale of either side is negative; the normalize is the walk's correctly rounded sqrt and division. Both operands are read from
 *      the INPUT row: no bone reads another bone's result. Without local_space, L = X.
 *      This is NOT the operand order of the reference's text: acl::object_to_local_space (compression/transform_pose_utils.h:59-74)
 *      writes qvv_normalize(qvv_mul(qvv_inverse(object[parent]), object[bone])). rtm::qvv_mul(lhs, rhs) applies lhs first and
 *      local_to_object_space computes qvv_mul(local, object[parent]), so its inverse is qvv_mul(object[bone], qvv_inverse(object[parent]))
 *      -- the order convert_to_relative has in the same tree (qvv_mul(transform, qvv_inverse(base))). Nothing in the reference calls
 *      object_to_local_space. Pushed back through local_to_object_space the order here returns the object pose to rounding (a few 1e-6
 *      relative); the reference's order is off by tens of units (tests/test_pose_buffer_inverse_oracle.py pins both). A launch that does
 *      not undo aclhip_transform_poses_batch is of no use, so the true inverse is what is built.
 *   2. With an additive format and base row Bs (the B records at base_poses + i * base_pose_stride_bytes), row i is per bone
 *      convert_to_relative (qvv_mul(L[b], qvv_inverse(Bs[b])), matrix route included), convert_to_additive0 (rotation quat_mul(L.rotation,
 *      conjugate(Bs.rotation)), translation L - Bs, scale L / Bs, the correctly rounded division) or convert_to_additive1 (rotation and
 *      translation alike, scale (L * (1 / Bs)) - 1) of (base = Bs[b], transform = L[b]), in exactly the reference's operation order.
 *      Nothing is normalized there and nothing is here. Otherwise row i is L.
 *   3. fp32, one IEEE operation at a time, never fused.
 *   4. The pads (the fourth float of a translation and of a scale): every record that went through step 1's product or through step 2
 *      is written with both pads 0. A root of a launch without an additive format keeps the bytes of X, pads included -- the rule of
 *      aclhip_transform_poses_batch.
 *   5. All B records are written; bytes of a row behind B * 48 are untouched.
 *   6. aclhip_get_negative_scale_count moves by one per qvv_mul that takes the matrix route: step 1's product and convert_to_relative's,
 *      as the forward launch counts its own.
 *   What undoes what: the launch undoes aclhip_transform_poses_batch -- local_space its object_space, format F its format F with the
 * same base -- up to rounding for unit rotations and ONE scale per bone (s, s, s), mirrored bones (-s, -s, -s) included. QVV transforms
 * are not closed under inversion when a scale is non-uniform: that is rtm::qvv_inverse, not a choice made here. A scale of 0 gives
 * infinities.
 *   In place: poses == source_poses with equal strides is allowed, and is the expected use -- a wave has its row complete in LDS before
 * it stores, and no wave reads another instance's row. Any other overlap of the output range with the source range, and any overlap of
 * the output range with the base range, is ACLHIP_ERROR_INVALID_ARGUMENT; the host decides this from the three (pointer, stride,
 * num_instances) ranges, [pointer, pointer + stride * num_instances).
 *   Refused and counted (aclhip_get_rejected_instance_count), the row untouched: an unknown or retired skeleton handle (0 included);
 * local_space on a skeleton without hierarchy; B * 48 larger than any of the strides in use (source_pose_stride_bytes,
 * pose_stride_bytes, base_pose_stride_bytes with an additive format); B beyond the launch's LDS image. The refusal comes in front of any
 * load of a row: no instance reads or writes outside its rows, whatever instance_skeletons holds. A skeleton unregistered after the
 * launch was enqueued is still served.
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): inverse == NULL,
 * source_poses == NULL or poses == NULL; no skeleton at all (skeleton == 0 and instance_skeletons == NULL); local_space == 0 with
 * ACLHIP_ADDITIVE_NONE (nothing to do); an unknown format; a format other than NONE without base_poses, or the reverse; pointers or
 * strides that are not 16 byte aligned; reserved fields that are not 0; a shape that does not fit 160 KiB of LDS; the overlaps above.
 *   The launch's shape comes from pose_stride_bytes / 48 alone (slots per LDS image). Registered clips play no part. The launch goes on
 * `stream`, can be captured into a graph, and uploads nothing.
 *   Out of scope (nothing here precludes them): bounds; blend masks or strengths; QVV40 / QV32 rows; ACLHIP_CONSUMERS_FAST; the host
 * convenience form; the C++ mirror in aclhip.hpp; instance lists.
 *   What it costs (one MI355X, 65 536 x 100 bones, medians of three interleaved rounds of 20 launches): local_space 107 us out of place
 * and 108 us in place, local_space plus relative 165 us for 1.5 x the bytes, against 121 us (112 - 141 over its three rounds) for
 * aclhip_transform_poses_batch with object space on the same buffers in the same rounds: no slower than the forward launch, 0.72 - 0.74
 * of the HBM peak (tools/pose_buffer_inverse.py, profiles/pose_buffer_inverse.md; DESIGN.md 4.7 "Inverse pose buffers"). */
aclhip_status aclhip_inverse_transform_poses_batch(aclhip_context* context, const void* source_poses, uint64_t source_pose_stride_bytes,
	uint32_t num_instances, const aclhip_pose_buffer_inverse* inverse, void* poses, uint64_t pose_stride_bytes, void* stream);

/* ---- pose error: how far two pose buffers are apart, measured on a shell around every bone ----------
 * The other consumer of a decoded pose in the reference is its error measure: acl::calculate_compression_error
 * (compression/track_error.h, impl/track_error.impl.h:219-387) decodes every sample of a clip twice, raw and lossy, takes both poses to
 * object space and asks qvvf_transform_error_metric::calculate_error (compression/transform_error_metrics.h:335-358) per bone how far
 * three virtual vertices at the bone's shell_distance moved; the worst bone of the worst sample is the track_error acl_compressor prints.
 * aclhip_measure_pose_error_batch is that measure over two pose buffers the caller filled -- two decodes of a clip, a pose before and
 * after an IK pass, a full and a stripped database tier -- with an 8 byte record per instance and, on request, every bone's error and the
 * worst record of the launch. (ABI version 6 still: added structs and an added function, no existing struct changed.) */
typedef struct aclhip_pose_error { float error; uint32_t bone; } aclhip_pose_error;		/* 8 bytes */
typedef struct aclhip_pose_error_worst { float error; uint32_t bone; uint32_t instance; uint32_t reserved; } aclhip_pose_error_worst;	/* 16 bytes */
#define ACLHIP_NO_BONE 0xFFFFFFFFu

typedef struct aclhip_pose_error_desc
{
	aclhip_skeleton skeleton;					/*  0  for every instance when instance_skeletons is NULL */
	const aclhip_skeleton* instance_skeletons;	/*  8  DEVICE [num_instances] or NULL */
	uint32_t object_space;						/* 16  1: both poses through local_to_object_space first (the reference's measure); 0: local space error */
	uint32_t additive_format;					/* 20  aclhip_additive_format; NONE: no base buffer */
	const void* base_poses;						/* 24  DEVICE or NULL: QVV48, skeleton order, local space */
	uint64_t base_pose_stride_bytes;			/* 32 */
	const float* shell_distances;				/* 40  DEVICE [num_shell_distances] or NULL: one per bone, shared by the launch */
	uint32_t num_shell_distances;				/* 48 */
	float shell_distance;						/* 52  for every bone when shell_distances is NULL */
	float* bone_errors;							/* 56  DEVICE or NULL: error of bone b of instance i at (char*)bone_errors + i * bone_error_stride_bytes + 4 * b */
	uint64_t bone_error_stride_bytes;			/* 64 */
	aclhip_pose_error_worst* worst;				/* 72  DEVICE or NULL: one record for the launch */
	uint64_t reserved[2];						/* 80  0 */
} aclhip_pose_error_desc;						/* 96 bytes */

/* The definition. Instance i has skeleton S (desc->skeleton, or instance_skeletons[i]) with B bones and parents P; R and Y are the B QVV48
 * records at raw_poses + i * raw_pose_stride_bytes and lossy_poses + i * lossy_pose_stride_bytes.
 *   1. With an additive format and base row Bs (the B records at base_poses + i * base_pose_stride_bytes):
 *      R'[b] = apply_additive_to_base(format, base = Bs[b], additive = R[b]), and Y' from Y alike -- the roles of
 *      track_error.impl.h:351-352, the arithmetic of aclhip_transform_poses_batch's step 2. Otherwise R' = R and Y' = Y.
 *   2. With object_space: Ro = local_to_object_space(P, R') and Yo = local_to_object_space(P, Y'), bit for bit what
 *      aclhip_transform_poses_batch would write for that buffer: the same walk, rtm::qvv_mul's matrix route where a scale of either side
 *      is negative, the correctly rounded normalize (short_exact 0); aclhip_get_negative_scale_count moves as it would for those two
 *      launches (steps 1 and 2). Otherwise Ro = R' and Yo = Y'.
 *   3. The error of bone b, with d = shell_distances[b], or shell_distance when the table is NULL, and the three points p_0 = (d, 0, 0),
 *      p_1 = (0, d, 0), p_2 = (0, 0, d) (transform_error_metrics.h:335-358):
 *        point(p, t) = quat_mul_vector3(t.scale * p, t.rotation) + t.translation            rtm::qvv_mul_point3; quat_mul_vector3(v, q) =
 *                      quat_mul(quat_mul(conjugate(q), (v, 0)), q), the function the inverse launch uses for a translation
 *        e_k         = sqrt((dx * dx + dy * dy) + dz * dz) with (dx, dy, dz) = point(p_k, Yo[b]) - point(p_k, Ro[b])
 *        error[b]    = max(max(e_0, e_1), e_2) with max(a, b) = a > b ? a : b
 *      fp32, one IEEE operation at a time, never fused, the correctly rounded sqrt; all three components of t.scale * p are multiplied,
 *      the zero ones too.
 *   4. errors[i] is the scan of track_error.impl.h:358-375: it starts from { -1, ACLHIP_NO_BONE }, walks the bones in ascending order and
 *      takes bone b when error[b] > the record's error. A NaN never wins; ties go to the lowest bone; with B = 0, or with every error a
 *      NaN, the record stays { -1, ACLHIP_NO_BONE } -- the reference's invalid_track_error.
 *   5. With bone_errors: error[b] is stored for every b < B, a NaN as a NaN (its payload is not specified); bytes of the row behind 4 * B
 *      are untouched.
 *   6. With worst: the one record of the launch is the same scan over errors[0 .. num_instances) in ascending instance order -- the
 *      greatest error, its bone, the lowest instance that has it; { -1, ACLHIP_NO_BONE, 0xFFFFFFFF, 0 } when no instance has an error
 *      >= 0, num_instances == 0 included. It is deterministic and written by the call itself, stream ordered (a second launch of one
 *      workgroup over the records): the caller initialises nothing.
 *   Against the reference itself: identical, but for its x86 normalize in the walk, which starts from the reciprocal square root estimate
 *   and so differs from the correctly rounded one by a few ulp per level of the hierarchy (the CPU oracle the tests compare with
 *   says the same of its local_to_object_space). That difference is stated here and not tested.
 *   Refused and counted (aclhip_get_rejected_instance_count): an unknown or retired skeleton handle (0 included); object_space on a
 * skeleton without hierarchy; B * 48 larger than any stride in use (raw, lossy, base with an additive format); 4 * B larger than
 * bone_error_stride_bytes; B larger than num_shell_distances when the table is given; B beyond the launch's LDS images. A refused
 * instance's errors[i] IS written, as { -1, ACLHIP_NO_BONE }: unlike a pose row this record says "not measured", and the worst scan skips
 * it by its sign. Its bone_errors row is untouched. The refusal comes in front of any load of a row.
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): desc, raw_poses,
 * lossy_poses or errors == NULL; no skeleton at all; an unknown format; a format other than NONE without base_poses, or the reverse;
 * shell_distances with num_shell_distances == 0; bone_errors with a stride that is 0 or no multiple of 4; pointers or strides of pose
 * rows that are not 16 byte aligned; errors not 8 byte aligned; worst not 16 byte aligned; reserved fields that are not 0; a shape that
 * does not fit 160 KiB of LDS; any output range (errors, bone_errors, worst) that overlaps an input range or another output. raw, lossy
 * and base are only read and may overlap each other freely: the same buffer twice gives error 0 and bone 0.
 *   The launch's shape comes from min(raw_pose_stride_bytes, lossy_pose_stride_bytes) / 48 (slots per LDS image, two images per
 * instance). Registered clips play no part. The launch goes on `stream`, can be captured into a graph, and uploads nothing.
 *   Out of scope (nothing here precludes them): the _no_scale variants; a decode fused into the measure; QVV40 / QV32 rows; the C++
 * mirror in aclhip.hpp; instance lists. (qvvf_matrix3x4f_transform_error_metric is aclhip_measure_pose_error_metric_batch, below.)
 *   What it costs (one MI355X, 65 536 x 100 bones, object space, medians of three interleaved rounds of 20 launches): 293 us for the
 * records alone, 309 us with the worst record, 311 us with every bone's error as well, against 222 us for the two
 * aclhip_transform_poses_batch object space launches on the same two buffers in the same rounds -- 1.32 to 1.40 x what a caller pays
 * today before it has compared anything, and nothing is copied to the host. The launch moves two row reads and 8 bytes per instance
 * out, 630 MB: 2.1 TB/s, 0.27 of the HBM peak, so its reads do not bound it; no counter run has been taken yet
 * (tools/pose_error.py, profiles/pose_error.md; DESIGN.md 4.7 "Pose error"). */
aclhip_status aclhip_measure_pose_error_batch(aclhip_context* context, const void* raw_poses, uint64_t raw_pose_stride_bytes,
	const void* lossy_poses, uint64_t lossy_pose_stride_bytes, uint32_t num_instances, const aclhip_pose_error_desc* desc,
	aclhip_pose_error* errors /* DEVICE [num_instances], required */, void* stream);

/* ---- matrix object space: 3x4 pose matrices and the matrix3x4f error metric -------------------------
 * Everything above works in rtm::qvvf. The reference has a second arithmetic: qvvf_matrix3x4f_transform_error_metric
 * (compression/transform_error_metrics.h:389-462) converts every local transform with rtm::matrix_from_qvv, walks the hierarchy with
 * rtm::matrix_mul and measures with rtm::matrix_mul_point3. It is the metric the reference names for clips with scale: a QVV product
 * cannot hold the shear a non-uniform parent scale puts on a rotated child, so for such rigs the QVV object space pose is not the pose the
 * renderer draws. aclhip_pose_matrices_batch writes those matrices -- what leaves an animation system for the renderer -- from a pose
 * buffer the caller filled, and aclhip_measure_pose_error_metric_batch measures two pose buffers in that arithmetic. (ABI version 6
 * still: an added struct, two added enums and two added functions, no existing struct changed.) */
typedef enum aclhip_matrix_layout
{
	ACLHIP_MATRIX_3X4F_64 = 0		/* rtm::matrix3x4f: x_axis | y_axis | z_axis | w_axis, four floats each, 64 bytes per bone */
} aclhip_matrix_layout;

typedef struct aclhip_pose_matrices_desc
{
	aclhip_skeleton skeleton;					/*  0  for every instance when instance_skeletons is NULL */
	const aclhip_skeleton* instance_skeletons;	/*  8  DEVICE [num_instances] or NULL */
	uint32_t object_space;						/* 16  1: the matrix walk; 0: convert_transforms alone */
	uint32_t layout;							/* 20  aclhip_matrix_layout */
	uint64_t reserved[2];						/* 24  0 */
} aclhip_pose_matrices_desc;					/* 40 bytes */

/* The definition. Instance i has skeleton S (desc->skeleton, or instance_skeletons[i]) with B bones and parents P; L is the B QVV48
 * records at local_poses + i * local_pose_stride_bytes.
 *   1. M[b] = matrix_from_qvv(L[b]) (rtm::matrix_from_qvv, in the operation order the tests' CPU restatement spells out), with
 *      (x, y, z, w) the rotation: x2 = x + x, y2 = y + y, z2 = z + z; xx = x * x2, xy = x * y2, xz = x * z2, yy = y * y2, yz = y * z2, zz = z * z2,
 *      wx = w * x2, wy = w * y2, wz = w * z2;
 *        x_axis = (1 - (yy + zz), xy + wz, xz - wy) * scale.x
 *        y_axis = (xy - wz, 1 - (xx + zz), yz + wx) * scale.y
 *        z_axis = (xz + wy, yz - wx, 1 - (xx + yy)) * scale.z
 *        w_axis = translation
 *   2. With object_space: a root keeps M; every other bone is O[b] = matrix_mul(M[b], O[P[b]]), lhs first -- the metric's
 *      local_to_object_space (transform_error_metrics.h:415-436). With R = O[P[b]] and v one of the three axis rows of M[b], the row of
 *      O[b] is ((R.x_axis * v.x) + R.y_axis * v.y) + R.z_axis * v.z per component; the w row is the same with v = M[b].w_axis, plus
 *      R.w_axis, added last. Without object_space O = M (the metric's convert_transforms alone).
 *   3. Row i of `matrices` (at matrices + i * matrix_stride_bytes) gets B records of 64 bytes, x_axis | y_axis | z_axis | w_axis: the
 *      three components of each axis in lanes 0-2; lane 3 is written as +0 for the three axes and 1.0f for w_axis, whatever the inputs
 *      held -- the fourth lane is no part of a 3x4 matrix's value. Bytes of a row behind 64 * B are untouched.
 *   fp32, one IEEE operation at a time, never fused. Nothing is assumed about a caller's rotations or scales: nothing is normalized, and a
 *   NaN or an infinity propagates to the bone and its descendants and nowhere else. There is no rtm::qvv_mul here:
 *   aclhip_get_negative_scale_count does not move.
 *   Refused and counted (aclhip_get_rejected_instance_count), the row untouched, decided in front of any load of a row: an unknown or
 * retired skeleton handle (0 included); object_space on a skeleton without hierarchy; B * 48 > local_pose_stride_bytes; B * 64 >
 * matrix_stride_bytes; B beyond the launch's LDS image.
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): desc, local_poses or
 * matrices == NULL; no skeleton at all; an unknown layout; pointers or strides that are not 16 byte aligned; reserved fields that are not
 * 0; a shape that does not fit the LDS; ANY overlap of the output range with the input range -- records differ in size, so there is no in
 * place form.
 *   The launch's shape comes from min(local_pose_stride_bytes / 48, matrix_stride_bytes / 64) slots per LDS image. Registered clips play
 * no part. The launch goes on `stream`, can be captured into a graph, and uploads nothing.
 *   Out of scope (nothing here precludes them): an additive buffer in the matrix launch (chain aclhip_transform_poses_batch in local
 * space first); bounds; the _no_scale variants; a decode fused into either launch; QVV40 / QV32 rows; instance lists; the C++ mirror in
 * aclhip.hpp. (A 48 byte transposed layout and inverse bind matrices: aclhip_skinning_matrices_batch, below.)
 *   What it costs (one MI355X, 65 536 x 100 bones, object space; tools/pose_matrices.py, profiles/pose_matrices.md, DESIGN.md 4.7 "Pose
 * matrices"): 129.8 us next to 109.6 us of aclhip_transform_poses_batch with object space from the same buffer -- 1.18 x the time for
 * 1.17 x the bytes, both at 0.71 of the HBM peak. */
aclhip_status aclhip_pose_matrices_batch(aclhip_context* context, const void* local_poses, uint64_t local_pose_stride_bytes,
	uint32_t num_instances, const aclhip_pose_matrices_desc* desc, void* matrices, uint64_t matrix_stride_bytes, void* stream);

typedef enum aclhip_error_metric
{
	ACLHIP_METRIC_QVVF = 0,				/* qvvf_transform_error_metric: aclhip_measure_pose_error_batch itself */
	ACLHIP_METRIC_QVVF_MATRIX3X4F = 1	/* qvvf_matrix3x4f_transform_error_metric */
} aclhip_error_metric;

/* aclhip_measure_pose_error_batch with the error metric as an argument: the same desc, the same records, the same bone_errors and worst,
 * the same refusals and argument checks.
 *   ACLHIP_METRIC_QVVF is aclhip_measure_pose_error_batch: one host path, the same kernel, the same bits.
 *   ACLHIP_METRIC_QVVF_MATRIX3X4F: steps 1 and 2 of that definition are replaced by steps 1 and 2 of aclhip_pose_matrices_batch, applied to
 * both rows (with object_space == 0 the conversion alone), and step 3 by the metric's calculate_error (transform_error_metrics.h:438-461):
 *        point(p, T) = (((T.x_axis * p.x) + T.y_axis * p.y) + T.z_axis * p.z) + T.w_axis       rtm::matrix_mul_point3; all three products
 *                      are made, the zero ones too
 *   with e_k, the max of three, the scan (step 4), bone_errors (step 5) and the worst record (step 6) unchanged. The negative scale counter
 *   does not move. additive_format != NONE is ACLHIP_ERROR_INVALID_ARGUMENT with a message: the reference's matrix metric inherits the
 *   QVV apply_additive_to_base and runs it over matrix buffers, so there is nothing defined to reproduce.
 *   An unknown metric is ACLHIP_ERROR_INVALID_ARGUMENT.
 *   What it costs (same batch; tools/pose_matrices.py, profiles/pose_matrices.md): the matrix metric 203.4 us next to 286.1 us of
 *   aclhip_measure_pose_error_batch over the same two buffers, 0.39 of the HBM peak. */
aclhip_status aclhip_measure_pose_error_metric_batch(aclhip_context* context, const void* raw_poses, uint64_t raw_pose_stride_bytes,
	const void* lossy_poses, uint64_t lossy_pose_stride_bytes, uint32_t num_instances, const aclhip_pose_error_desc* desc, uint32_t metric,
	aclhip_pose_error* errors /* DEVICE [num_instances], required */, void* stream);

/* ---- skinning palettes: inverse bind matrices times object matrices, per mesh joint ------------------
 * A renderer does not skin with the object space matrices of the bones: it skins with a PALETTE -- per mesh joint j the matrix
 * inverse_bind[j] * object[bone_of_joint[j]], usually packed as three float4 rows (48 bytes). aclhip_skinning_matrices_batch is
 * aclhip_pose_matrices_batch with that product and that packing in the place of its store: the object matrices never reach HBM, and a
 * caller needs no kernel of its own between the pose buffer and the draw. (ABI version 6 still: two added structs, an added enum and five
 * added functions, no existing struct changed.)
 *
 * A SKIN is what a mesh brings to a skeleton (glTF skin.joints + inverseBindMatrices, an FBX cluster list): num_joints palette entries,
 * for each the skeleton bone it follows and its inverse bind matrix.
 * aclhip_register_skin: `joint_bones` (HOST, num_joints entries, each < num_bones; NULL: the identity list, and then num_joints ==
 * num_bones is required; duplicates are allowed -- two joints may follow one bone, so num_joints may exceed num_bones); `inverse_bind`
 * (HOST, num_joints records in the ACLHIP_MATRIX_3X4F_64 layout -- 16 floats, x_axis | y_axis | z_axis | w_axis, what
 * aclhip_pose_matrices_batch writes: a caller can make the bind pose's object matrices with that call and invert them on the host; lane 3
 * of every axis is ignored; NULL: identity matrices). Refused with ACLHIP_ERROR_INVALID_ARGUMENT before any device call (the message
 * names the first offending joint): num_joints == 0 or > 0xFFFF; num_bones == 0 or > 0xFFFF; a joint bone >= num_bones; a matrix
 * component (lanes 0-2) that is not finite; NULL joint_bones with num_joints != num_bones. Lifetime is a blend mask's: the device table
 * (ACLHIP_MAX_SKINS records) is allocated at the first registration and never moves, so a captured hipGraph that names a skin stays valid
 * while others come and go; handle 0 is null; uploads go on the context's own stream; unregistration is stream ordered (launches already
 * enqueued still see the skin, later ones refuse it) and nobody waits. */
typedef uint32_t aclhip_skin;				/* handle returned by aclhip_register_skin; 0 = none */
#define ACLHIP_MAX_SKINS 4096u				/* live skins of one context, the null handle included */

typedef struct aclhip_skin_info
{
	uint32_t num_joints;
	uint32_t num_bones;						/* the skeleton size the skin was made for */
	uint32_t is_identity_joint_list;		/* num_joints == num_bones and joint_bones[j] == j */
	uint32_t has_inverse_bind;				/* 0: registered with NULL (identity matrices) */
	uint32_t reserved[4];
} aclhip_skin_info;

/* Host only (no context, no device): what registration checks and what aclhip_get_skin_info reports. `message` (may be NULL,
 * `message_capacity` bytes) receives the reason when the skin is refused; `out_info` may be NULL. */
aclhip_status aclhip_check_skin(const uint32_t* joint_bones, const float* inverse_bind, uint32_t num_joints, uint32_t num_bones,
	aclhip_skin_info* out_info, char* message, uint32_t message_capacity);

aclhip_status aclhip_register_skin(aclhip_context* context, const uint32_t* joint_bones, const float* inverse_bind, uint32_t num_joints,
	uint32_t num_bones, aclhip_skin* out_skin);
aclhip_status aclhip_unregister_skin(aclhip_context* context, aclhip_skin skin);
aclhip_status aclhip_get_skin_info(const aclhip_context* context, aclhip_skin skin, aclhip_skin_info* out_info);

typedef enum aclhip_palette_layout
{
	ACLHIP_PALETTE_3X4F_64 = 0,				/* rtm::matrix3x4f, as aclhip_pose_matrices_batch writes it: lane 3 = 0, 0, 0, 1 */
	ACLHIP_PALETTE_3X4F_TRANSPOSED_48 = 1	/* three float4 rows r_k = (x_axis[k], y_axis[k], z_axis[k], w_axis[k]), k = 0, 1, 2:
											 * p' = (dot(r_0, (p, 1)), dot(r_1, (p, 1)), dot(r_2, (p, 1))) -- an HLSL float3x4, three texel fetches */
} aclhip_palette_layout;

typedef struct aclhip_skinning_desc
{
	aclhip_skeleton skeleton;					/*  0  for every instance when instance_skeletons is NULL */
	const aclhip_skeleton* instance_skeletons;	/*  8  DEVICE [num_instances] or NULL */
	aclhip_skin skin;							/* 16  for every instance when instance_skins is NULL */
	const aclhip_skin* instance_skins;			/* 24  DEVICE [num_instances] or NULL */
	uint32_t object_space;						/* 32  1: the matrix walk over local rows; 0: the rows are taken as they are (already object space) */
	uint32_t layout;							/* 36  aclhip_palette_layout */
	uint64_t reserved[2];						/* 40  0 */
} aclhip_skinning_desc;							/* 56 bytes */

/* The definition. Instance i has skeleton S (desc->skeleton, or instance_skeletons[i]) with B bones and skin K (desc->skin, or
 * instance_skins[i]) with J joints, bones k[j] and inverse bind matrices IB[j]; L is the B QVV48 records at poses + i * pose_stride_bytes.
 *   1. O = steps 1 and 2 of aclhip_pose_matrices_batch over L: M[b] = matrix_from_qvv(L[b]) and, with object_space, O[b] =
 *      matrix_mul(M[b], O[P[b]]) for every bone that has a parent; without it O = M. Bit for bit what that launch would store.
 *   2. S[j] = matrix_mul(IB[j], O[k[j]]), lhs first, in the operation order of step 2 there: with R = O[k[j]] and v one of the three axis
 *      rows of IB[j], the row of S[j] is ((R.x_axis * v.x) + R.y_axis * v.y) + R.z_axis * v.z per component; the w row is the same with v =
 *      IB[j].w_axis, plus R.w_axis, added last. fp32, one IEEE operation at a time, never fused. The product is made with identity
 *      matrices too (a skin registered with NULL): a NaN or an infinity of bone k[j] reaches joint j, and no other joint.
 *   3. Row i of `palettes` (at palettes + i * palette_stride_bytes) gets J records. ACLHIP_PALETTE_3X4F_64: 64 bytes, x_axis | y_axis |
 *      z_axis | w_axis of S[j] with lane 3 written as +0, +0, +0, 1.0f. ACLHIP_PALETTE_3X4F_TRANSPOSED_48: 48 bytes, the three rows
 *      r_k = (S[j].x_axis[k], S[j].y_axis[k], S[j].z_axis[k], S[j].w_axis[k]); there is no spare lane. Bytes of a row behind the J
 *      records are untouched.
 *   Nothing is normalized and there is no rtm::qvv_mul here: aclhip_get_negative_scale_count does not move.
 *   Refused and counted (aclhip_get_rejected_instance_count), the row untouched, decided in front of any load of a row: an unknown or
 * retired skeleton or skin handle (0 included); a skin whose num_bones differs from the skeleton's; object_space on a skeleton without
 * hierarchy; B * 48 > pose_stride_bytes; J * (64 or 48) > palette_stride_bytes; B beyond the launch's LDS image.
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): desc, poses or
 * palettes == NULL; no skeleton at all; no skin at all; an unknown layout; pointers or strides that are not 16 byte aligned; reserved
 * fields that are not 0; a shape that does not fit the LDS; ANY overlap of the output range with the input range (the pose rows, the
 * skeleton list, the skin list) -- there is no in place form.
 *   The launch's shape comes from pose_stride_bytes / 48 slots per LDS image. Registered clips play no part. The launch goes on `stream`,
 * can be captured into a graph, and uploads nothing.
 *   Out of scope (nothing here precludes them): computing inverse bind matrices on the device; bounds; a decode fused into the launch;
 * QVV40 / QV32 rows; dual quaternions; the C++ mirror in aclhip.hpp.
 *   What it costs (one MI355X, 65 536 x 100 bones, a skin of 100 joints, object space, medians of three interleaved rounds of 20 launches;
 * tools/skinning_matrices.py, profiles/skinning_matrices.md, DESIGN.md 4.7 "Skinning matrices"): 166.3 us for the transposed layout and
 * 186.9 us for the 64 byte layout next to 130.9 us of aclhip_pose_matrices_batch with object space from the same buffer in the same
 * rounds -- 1.27 x and 1.43 x its time for 0.86 x and 1.00 x its bytes, 0.47 and 0.49 of the HBM peak against its 0.70: the launch is not
 * priced by its bytes yet; the one storing wave's dependent loads per joint are the suspect, and no counter run has been taken. */
aclhip_status aclhip_skinning_matrices_batch(aclhip_context* context, const void* poses, uint64_t pose_stride_bytes, uint32_t num_instances,
	const aclhip_skinning_desc* desc, void* palettes, uint64_t palette_stride_bytes, void* stream);

/* ---- raw track arrays: batched sample_tracks of uncompressed clips -----------------------------------
 * Every other pose here starts from a compressed_tracks blob. A RAW TRACK ARRAY is the reference's second source of poses, an
 * UNCOMPRESSED clip -- acl::track_array_qvvf (compression/track_array.h) -- and aclhip_sample_raw_tracks_batch is its sample_tracks
 * (compression/impl/track_array.impl.h:209-343) over a batch: the raw side of calculate_compression_error, and the way mocap takes under
 * review, replays being recorded, procedural clips and clips queued for compression join a batch whose other rows are decoded. (ABI
 * version 6 still: two added structs and five added functions, no existing struct changed.)
 *
 * aclhip_register_raw_tracks: `samples` is a HOST array of [num_samples][num_tracks] QVV48 records (rotation xyzw | translation xyz, any
 * | scale xyz, any), SAMPLE MAJOR: one key frame of the whole pose is one contiguous run. The caller may free it when the call returns.
 * The device image keeps that layout; the fourth lanes of translations and scales are kept as given and no kernel reads them.
 * `looping_policy` is ACLHIP_LOOP_CLAMP or ACLHIP_LOOP_WRAP (track_array::set_looping_policy takes nothing else either, :126-133);
 * the array's duration is calculate_finite_duration(num_samples + (wrap ? 1 : 0), sample_rate) (track_array::get_finite_duration,
 * :113-124), computed on the host. Refused with ACLHIP_ERROR_INVALID_ARGUMENT and a message, before any device call: samples or out_raw
 * == NULL; num_tracks == 0 or > 0xFFFF; num_samples == 0; num_samples * num_tracks * 48 >= 2^31; a sample_rate that is not finite or
 * not > 0; ACLHIP_LOOP_AS_COMPRESSED or an unknown policy. VALUES ARE NOT CHECKED: a NaN in a key frame reaches the tracks that read it,
 * and no others. Lifetime is a skin's: the device table (ACLHIP_MAX_RAW_TRACKS records) is allocated at the first registration and never
 * moves, so a captured hipGraph that names an array stays valid while others come and go; handle 0 is null; uploads go on the context's
 * own stream; unregistration is stream ordered (launches already enqueued still see the array, later ones refuse it) and nobody waits. */
typedef uint32_t aclhip_raw_tracks;			/* handle returned by aclhip_register_raw_tracks; 0 = none */
#define ACLHIP_MAX_RAW_TRACKS 4096u			/* live arrays of one context, the null handle included */

typedef struct aclhip_raw_tracks_info
{
	uint32_t num_tracks;
	uint32_t num_samples;
	float sample_rate;
	float duration;							/* track_array::get_finite_duration() */
	uint32_t looping_policy;				/* ACLHIP_LOOP_CLAMP or ACLHIP_LOOP_WRAP */
	uint32_t reserved[3];
} aclhip_raw_tracks_info;

/* Host only (no context, no device): what registration checks and what aclhip_get_raw_tracks_info reports; `samples` is only tested
 * against NULL. `message` (may be NULL, `message_capacity` bytes) receives the reason when the array is refused; `out_info` may be NULL. */
aclhip_status aclhip_check_raw_tracks(const void* samples, uint32_t num_tracks, uint32_t num_samples, float sample_rate,
	uint32_t looping_policy, aclhip_raw_tracks_info* out_info, char* message, uint32_t message_capacity);

aclhip_status aclhip_register_raw_tracks(aclhip_context* context, const void* samples, uint32_t num_tracks, uint32_t num_samples,
	float sample_rate, uint32_t looping_policy, aclhip_raw_tracks* out_raw);
aclhip_status aclhip_unregister_raw_tracks(aclhip_context* context, aclhip_raw_tracks raw);
aclhip_status aclhip_get_raw_tracks_info(const aclhip_context* context, aclhip_raw_tracks raw, aclhip_raw_tracks_info* out_info);

typedef struct aclhip_raw_sample_desc
{
	uint8_t rounding_policy;					/*  0  aclhip_rounding_policy for every instance; ROUND_PER_TRACK needs track_rounding_policies */
	uint8_t reserved0[7];
	const uint8_t* instance_rounding_policies;	/*  8  DEVICE [num_instances] or NULL: overrides rounding_policy */
	const uint8_t* track_rounding_policies;		/* 16  DEVICE [num_track_rounding_policies] or NULL: track_writer::get_rounding_policy per track,
												       read for an instance whose policy is PER_TRACK; an entry is NONE/FLOOR/CEIL/NEAREST */
	uint32_t num_track_rounding_policies;		/* 24 */
	uint32_t reserved1;
	const uint32_t* rows;						/* 32  DEVICE [num_instances] distinct rows, or NULL: row i */
	uint64_t reserved[2];						/* 40  0 */
} aclhip_raw_sample_desc;						/* 56 bytes */

/* The definition. All arithmetic is fp32, one IEEE operation at a time, never fused. Instance i has array A = raws[i] with T tracks, S
 * samples, rate r, looping policy L and duration D, and rounding policy p = instance_rounding_policies[i], or desc->rounding_policy (a
 * device value above PER_TRACK is taken as NONE).
 *   1. t = min(max(sample_times[i], 0), D); (k0, k1, alpha) = find_linear_interpolation_samples_with_sample_rate(S, r, t, per_track, L)
 *      (core/impl/interpolation_utils.impl.h:143-201): the two key frames and the UNROUNDED alpha = t * r - k0 (k0 = k1 = 0 and alpha = 0
 *      when a wrapped t * r lands behind the last sample). A NaN sample time is not specified (nothing is read outside the array).
 *   2. Per track b < T: q = p, or track_rounding_policies[b] when p is PER_TRACK; a_b = apply_rounding_policy(alpha, q) (:261-278): alpha,
 *      0, 1, or floor(alpha + 0.5).
 *   3. With V0, V1 the records of track b at key frames k0, k1:
 *        rotation    = quat_normalize(quat_lerp_no_normalization(V0.rotation, V1.rotation, a_b)): dot = ((x0 * x1 + y0 * y1) + z0 * z1) +
 *                      w0 * w1 accumulated in that order, V1's components get the dot's sign bit flipped in, each component is
 *                      (end * a_b) + (start - (start * a_b)); then n = ((x * x + y * y) + z * z) + w * w, the components times the
 *                      correctly rounded 1.0f / sqrtf(n) -- the general form for every input, denormal n included: nothing is proven about
 *                      a caller's rotations. The normalize runs for every policy (rtm::quat_lerp normalizes at alpha 0 and 1 too).
 *        translation, scale = (V1.x * a_b) + (V0.x - (V0.x * a_b)) per component (rtm::vector_lerp).
 *   4. Track b is stored at poses + row * pose_stride_bytes + 48 * b (row = rows[i], or i): rotation xyzw | translation xyz, +0 | scale
 *      xyz, +0. The fourth lanes are written as +0 whatever the key frames held, as the decode writes them. Bytes of a row behind 48 * T
 *      are untouched.
 *   Against the reference itself the results are identical but for rtm::quat_normalize's x86 reciprocal square root estimate, the
 * difference DESIGN.md 8 states for decompress_track: here the normalize is the correctly rounded one.
 *   Refused and counted (aclhip_get_rejected_instance_count), the row untouched, decided in front of any load of a key frame: an unknown
 * or retired handle (0 included); 48 * T > pose_stride_bytes; PER_TRACK with T > num_track_rounding_policies.
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): raws, sample_times or
 * poses == NULL; poses or pose_stride_bytes not 16 byte aligned; a rounding_policy above PER_TRACK; PER_TRACK without
 * track_rounding_policies; track_rounding_policies with a count of 0; reserved fields that are not 0; the output range (num_instances
 * rows from `poses`) overlapping raws, sample_times or any array of the desc.
 *   desc == NULL: ROUND_NONE, row i. The launch goes on `stream`, can be captured into a graph and uploads nothing; registered clips play
 * no part. The instance arrays are plain device arrays: a retired handle in them is refused by the kernel, not by the host.
 *   Out of scope (nothing here precludes them): remapped output bones (track_array's remap_output); sample_track, the single-track
 * form; QVV40 / QV32 rows; the C++ mirror in aclhip.hpp. (The scalar track types of track_array are the raw scalar track arrays, below.)
 *   What it costs: (one MI355X, 65 536 instances of one array of 100 tracks x 301 samples at uniformly drawn times, rows of 4 800 bytes,
 * medians of three interleaved rounds of 20 launches; tools/raw_tracks.py, profiles/raw_tracks.md, DESIGN.md 4.7 "Raw track arrays"):
 * 81.1 us next to 60.1 us of aclhip_decompress_tracks_batch of a compressed clip of the same shape at the same times in the same rounds
 * -- 1.35 x its time for the same rows, 0.49 of the HBM peak (315 MB of rows plus the array's 1.4 MB) against its 0.65; the rig shape,
 * 300 tracks: 215.4 us against 172.7 us, 0.55 against 0.68. The spread between rounds is 31 % here (the fastest round took 64.7 us)
 * against the decode's 14 %. What the counters show per launch: the waves are parked at a wait for 65 % of their cycles (the decode's:
 * 52 %), they issue 1.56 x the decode's vector instructions (every wave runs the rotation's square root and division for a third of its
 * lanes), and the vector cache waits for the L2 four times as long (two loads per store): a wave waits for its two loads, computes and
 * stores, five times in turn, with nothing of the next turn in flight. NOT BUILT: the next turn's loads issued ahead of the arithmetic. */
aclhip_status aclhip_sample_raw_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	const float* sample_times /* DEVICE [num_instances] */, uint32_t num_instances, const aclhip_raw_sample_desc* desc, void* poses,
	uint64_t pose_stride_bytes, void* stream);

/* ---- raw scalar track arrays: batched sample_tracks / sample_track of uncompressed curve sets, and the scalar track error ------------
 * acl::track_array holds five more track types than qvvf: float1f, float2f, float3f, float4f and vector4f (compression/track_array.h).
 * A RAW SCALAR TRACK ARRAY is such an uncompressed curve set -- blend shape weights, material and camera curves, recorded or procedural
 * curves, curves queued for compression --, aclhip_sample_raw_scalar_tracks_batch is its sample_tracks
 * (compression/impl/track_array.impl.h:209-343) over a batch, aclhip_sample_raw_scalar_track_batch its sample_track (:345-438), and
 * aclhip_measure_scalar_error_batch is calculate_scalar_track_error (compression/impl/track_error.impl.h:53-103, :166-217) over two value
 * buffers: what the reference's scalar overloads of calculate_compression_error run for everything but qvvf. (ABI version 6 still: added
 * structs and added functions, no existing struct changed.)
 *
 * aclhip_register_raw_scalar_tracks: `samples` is a HOST array of [num_samples][num_tracks][C] floats, SAMPLE MAJOR and tight: one key
 * frame of the whole list is one contiguous run, laid out like the row aclhip_decompress_scalar_tracks_batch writes. `track_type` is
 * acl::track_type8 as aclhip_clip_info::track_type reports it: 0 to 3 for float1f to float4f, 4 for vector4f; C is 1, 2, 3, 4, 4 in that
 * order. The caller may free the array when the call returns; the device image keeps the layout. Looping policy and duration are a raw
 * track array's: ACLHIP_LOOP_CLAMP or ACLHIP_LOOP_WRAP, calculate_finite_duration(num_samples + (wrap ? 1 : 0), sample_rate). Refused with
 * ACLHIP_ERROR_INVALID_ARGUMENT and a message, before any device call: everything aclhip_register_raw_tracks refuses (samples or out_raw
 * == NULL; num_tracks == 0 or > 0xFFFF; num_samples == 0; a sample_rate that is not finite or not > 0; ACLHIP_LOOP_AS_COMPRESSED or an
 * unknown policy), its size limit as num_samples * num_tracks * C * 4 >= 2^31, track type 12 (qvvf: that is a raw track array) and any
 * unknown track type. VALUES ARE NOT CHECKED. The handles are a table of their own (ACLHIP_MAX_RAW_SCALAR_TRACKS records): a raw track
 * handle names no scalar array and the reverse, whatever its value. Lifetime, stream ordered unregistration and graph safety are a raw
 * track array's. */
typedef uint32_t aclhip_raw_scalar_tracks;		/* handle returned by aclhip_register_raw_scalar_tracks; 0 = none */
#define ACLHIP_MAX_RAW_SCALAR_TRACKS 4096u		/* live arrays of one context, the null handle included */

typedef struct aclhip_raw_scalar_tracks_info
{
	uint32_t num_tracks;
	uint32_t num_samples;
	float sample_rate;
	float duration;							/* track_array::get_finite_duration() */
	uint32_t looping_policy;				/* ACLHIP_LOOP_CLAMP or ACLHIP_LOOP_WRAP */
	uint32_t track_type;					/* acl::track_type8: 0 .. 4 */
	uint32_t num_components;				/* C: floats per track, 1 .. 4 */
	uint32_t reserved;
} aclhip_raw_scalar_tracks_info;			/* 32 bytes */

/* Host only (no context, no device): what registration checks and what aclhip_get_raw_scalar_tracks_info reports; `samples` is only
 * tested against NULL. `message` (may be NULL, `message_capacity` bytes) receives the reason when the array is refused; `out_info` may be NULL. */
aclhip_status aclhip_check_raw_scalar_tracks(const void* samples, uint32_t track_type, uint32_t num_tracks, uint32_t num_samples,
	float sample_rate, uint32_t looping_policy, aclhip_raw_scalar_tracks_info* out_info, char* message, uint32_t message_capacity);

aclhip_status aclhip_register_raw_scalar_tracks(aclhip_context* context, const void* samples, uint32_t track_type, uint32_t num_tracks,
	uint32_t num_samples, float sample_rate, uint32_t looping_policy, aclhip_raw_scalar_tracks* out_raw);
aclhip_status aclhip_unregister_raw_scalar_tracks(aclhip_context* context, aclhip_raw_scalar_tracks raw);
aclhip_status aclhip_get_raw_scalar_tracks_info(const aclhip_context* context, aclhip_raw_scalar_tracks raw, aclhip_raw_scalar_tracks_info* out_info);

/* The definition of aclhip_sample_raw_scalar_tracks_batch; the desc is aclhip_raw_sample_desc, unchanged. All arithmetic is fp32, one
 * IEEE operation at a time, never fused. Instance i has array A = raws[i] with T tracks of C floats, S samples, rate r, looping policy L
 * and duration D, and rounding policy p = instance_rounding_policies[i], or desc->rounding_policy (a device value above PER_TRACK is
 * taken as NONE).
 *   1. t = min(max(sample_times[i], 0), D); (k0, k1, alpha) as in step 1 of aclhip_sample_raw_tracks_batch: the two key frames and the
 *      UNROUNDED alpha, k0 guarded by min(k0, S - 1). A NaN sample time is not specified (nothing is read outside the array).
 *   2. Per track b < T: q = p, or track_rounding_policies[b] when p is PER_TRACK; a_b = apply_rounding_policy(alpha, q).
 *   3. Per component c < C, with V0, V1 the values of track b at key frames k0, k1: value = (V1[c] * a_b) + (V0[c] - (V0[c] * a_b))
 *      (rtm::scalar_lerp and rtm::vector_lerp are this expression).
 *   4. Track b is stored as C floats at values + row * stride_bytes + 4 * C * b (row = rows[i], or i): the row layout of
 *      aclhip_decompress_scalar_tracks_batch, so a sampled row and a decoded row of the same list compare element for element. Nothing
 *      is padded or zero filled; bytes of the row behind 4 * C * T are untouched. Arrays of different types may share a launch: each row
 *      has its own array's shape.
 *   Against the reference itself the values are identical in every bit (the tests hold it through a precision 0 compression).
 *   Refused and counted (aclhip_get_rejected_instance_count), the row untouched, decided in front of any load of a key frame: an unknown
 * or retired handle (0 included); 4 * C * T > stride_bytes; PER_TRACK with T > num_track_rounding_policies.
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): raws, sample_times or
 * values == NULL; values or stride_bytes not 4 byte aligned, or a stride of 0; a rounding_policy above PER_TRACK; PER_TRACK without
 * track_rounding_policies; track_rounding_policies with a count of 0; reserved fields that are not 0; the output range (num_instances
 * rows from `values`) overlapping raws, sample_times or any array of the desc.
 *   desc == NULL: ROUND_NONE, row i. The launch goes on `stream`, can be captured into a graph and uploads nothing.
 *   The kernel has two paths. Row base, stride and T * C are only 4 byte aligned in general: the DWORD path gives every lane one float
 * of the row and serves every case. A wave whose row and whose two key frames all start on 16 byte boundaries -- decided per instance
 * from the addresses themselves -- takes the row's whole quads with 16 byte loads and stores, each float of a quad with its own
 * track's alpha, and the last T * C % 4 floats the dword way. The bits are the same on both paths.
 *   Out of scope (nothing here precludes them): track_array's remap_output and stripped tracks (output_index); per-instance shapes in the
 * measure; the C++ mirror in aclhip.hpp; the qvvf single-track form.
 *   What it costs: (one MI355X, 65 536 instances of one float1f array of 256 tracks x 120 samples -- the bench's scalar list shape -- at
 * uniformly drawn times, medians of three interleaved rounds of 20 launches; tools/raw_scalar_tracks.py, profiles/raw_scalar_tracks.md,
 * DESIGN.md 4.7 "Raw scalar track arrays"): rows of 1 024 bytes, base and stride 16 byte aligned (the 16 byte path): 18.9 us next to
 * 25.6 us of aclhip_decompress_scalar_tracks_batch of the reference-compressed clip of the same array at the same times in the same
 * rounds, 0.74 x its time, 0.45 of the HBM peak (67 MB of rows plus the array's 123 KB) against its 0.33, spread 11 %. The same rows on
 * the dword path (the lab library's ACLHIP_RAW_SCALAR_DWORD=1): 26.5 us, 1.07 x the decode: the 16 byte path buys 0.71 x. Rows of 1 028
 * bytes, only 4 byte aligned (three rows of four on the dword path): 36.5 us next to 28.9 us, 1.26 x -- both launches pay for rows that
 * share cache lines with their neighbours, this one more. The single-track launch: 3.5 us next to 3.7 us of
 * aclhip_decompress_scalar_track_batch for the same 65 536 requests. No counter run has been taken. */
aclhip_status aclhip_sample_raw_scalar_tracks_batch(aclhip_context* context, const aclhip_raw_scalar_tracks* raws /* DEVICE [num_instances] */,
	const float* sample_times /* DEVICE [num_instances] */, uint32_t num_instances, const aclhip_raw_sample_desc* desc, void* values,
	uint64_t stride_bytes, void* stream);

/* track_array::sample_track, the single-track form: request i writes the C floats of track track_indices[i] of array raws[i] at values +
 * row * stride_bytes. The policy is the launch's or the instance's, or track_rounding_policies[track] under PER_TRACK. The reference
 * hands the policy to the key frame search, which rounds the alpha with the same apply_rounding_policy: THE BITS ARE THOSE OF THE
 * WHOLE-LIST LAUNCH FOR THAT TRACK (steps 1 to 3 above), and the tests hold it.
 *   Refused and counted, the request's bytes untouched: an unknown or retired handle; track >= T; 4 * C > stride_bytes; PER_TRACK with
 * track >= num_track_rounding_policies.
 *   ACLHIP_ERROR_INVALID_ARGUMENT: as above, plus track_indices == NULL and the output range overlapping track_indices. */
aclhip_status aclhip_sample_raw_scalar_track_batch(aclhip_context* context, const aclhip_raw_scalar_tracks* raws /* DEVICE [num_instances] */,
	const float* sample_times /* DEVICE [num_instances] */, const uint32_t* track_indices /* DEVICE [num_instances] */, uint32_t num_instances,
	const aclhip_raw_sample_desc* desc, void* values, uint64_t stride_bytes, void* stream);

/* The scalar track error. The records are the pose error's, so that one worst scan serves both. */
typedef aclhip_pose_error aclhip_track_error;				/* { float error; uint32_t track; } -- the same 8 bytes (the field is named bone) */
typedef aclhip_pose_error_worst aclhip_track_error_worst;	/* { error, track, instance, reserved } -- the same 16 bytes */
#define ACLHIP_NO_TRACK 0xFFFFFFFFu

typedef struct aclhip_scalar_error_desc
{
	uint32_t num_tracks;						/*  0  T >= 1, for every instance */
	uint32_t num_components;					/*  4  C in 1 .. 4 */
	float* track_errors;						/*  8  DEVICE or NULL: error of track b of instance i at (char*)track_errors + i * track_error_stride_bytes + 4 * b */
	uint64_t track_error_stride_bytes;			/* 16 */
	aclhip_track_error_worst* worst;			/* 24  DEVICE or NULL: one record for the launch */
	uint64_t reserved[2];						/* 32  0 */
} aclhip_scalar_error_desc;						/* 48 bytes */

/* The definition (track_error.impl.h:53-103 and :198-213). R and Y are the T tracks of C floats at raw_values + i * raw_stride_bytes and
 * lossy_values + i * lossy_stride_bytes, tight.
 *   1. e_c = fabs(R[b][c] - Y[b][c]) for c < C (the reference's zeroed missing lanes cannot win against an error >= 0).
 *   2. error[b] is the greatest e_c with max(a, b) = a > b ? a : b, taken in ascending component order; it is a NaN if any e_c is a NaN
 *      (the reference leaves NaN handling to the host's SIMD max; this rule is this library's: stored as a NaN, never wins).
 *   3. errors[i] starts from { -1, ACLHIP_NO_TRACK } and takes track b, in ascending order, when error[b] > the record's error. A NaN
 *      never wins; ties go to the lowest track.
 *   4. With track_errors: every error[b] is stored, a NaN as a NaN (its payload is not specified); bytes behind 4 * T are untouched.
 *   5. With worst: step 6 of aclhip_measure_pose_error_batch word for word -- the scan of errors[0 .. num_instances) in ascending instance
 *      order; { -1, ACLHIP_NO_TRACK, 0xFFFFFFFF, 0 } when nothing was measured; written by the call itself, also for num_instances == 0.
 *   There is no handle and no hierarchy: nothing is refused per instance. ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call,
 * each with a message (with or without a context): desc, raw_values, lossy_values or errors == NULL; T == 0; C outside 1 .. 4; 4 * C * T
 * larger than either stride; track_errors with a stride that is 0, no multiple of 4, or < 4 * T; values or strides that are not 4 byte
 * aligned; errors not 8 byte aligned; worst not 16 byte aligned; reserved fields that are not 0; any output range (errors, track_errors,
 * worst) overlapping an input or another output. raw and lossy may be the same buffer: every error is 0 and the record names track 0.
 *   One wave per instance, a lane per track in turn, 8 bytes out per instance: not a kernel tuned for bandwidth, and not measured. */
aclhip_status aclhip_measure_scalar_error_batch(aclhip_context* context, const void* raw_values, uint64_t raw_stride_bytes,
	const void* lossy_values, uint64_t lossy_stride_bytes, uint32_t num_instances, const aclhip_scalar_error_desc* desc,
	aclhip_track_error* errors /* DEVICE [num_instances], required */, void* stream);

/* ---- compress_track_list for raw scalar track arrays ------------------------------------------------------------------------------------
 * acl::compress_track_list for float1f .. vector4f (compression/impl/compress.scalar.impl.h:65-269 and the files it calls), batched: a
 * registered raw scalar track array -- it already lives in HBM -- becomes a `compressed_tracks` blob there. THE BLOB IS BYTE FOR BYTE THE
 * REFERENCE'S for the same samples and settings, hash included; nothing rests on a tolerance, and the tests hold every byte.
 *   Instance i compresses array raws[i] into (char*)blobs + i * blob_stride_bytes; blobs and the stride are 16 byte aligned. The launch
 * writes every byte of [0, size) itself -- the zero padding between the sections and the 15 trailing zero bytes included -- and touches
 * nothing behind `size`. Handles may repeat; arrays of different types and shapes share a launch. results[i] says how it went. */
#define ACLHIP_COMPRESS_OPTIMIZE_LOOPS 1u      /* compression_settings::optimize_loops (default off) */

typedef struct aclhip_scalar_compress_desc
{
	float precision;                  /*  0  track_desc_scalarf::precision of every track when track_precisions is NULL (reference default 0.00001F) */
	uint32_t flags;                   /*  4  ACLHIP_COMPRESS_* */
	const float* track_precisions;    /*  8  DEVICE or NULL: precision of track b, shared by the launch (like track_rounding_policies) */
	uint32_t num_track_precisions;    /* 16 */
	uint32_t max_tracks;              /* 20  tracks the workspace was sized for; an instance with more is refused */
	void* workspace;                  /* 24  DEVICE, 16 byte aligned, aclhip_scalar_compress_workspace_bytes(num_instances, max_tracks) bytes */
	uint64_t reserved[2];             /* 32  0 */
} aclhip_scalar_compress_desc;        /* 48 bytes */

typedef struct aclhip_compress_result { uint32_t status; uint32_t size; } aclhip_compress_result;   /* 8 bytes */
#define ACLHIP_COMPRESS_OK 0u
#define ACLHIP_COMPRESS_NOT_FINITE 1u          /* the reference's "Some samples are not finite": size 0, row untouched */
#define ACLHIP_COMPRESS_REFUSED 2u             /* size 0, row untouched, counted by aclhip_get_rejected_instance_count */

/* Host only. The bound of a blob: 52 + align4(T) + 8 * C * T + 4 * C * T * S + 15 rounded up to 16 -- headers, per-track metadata, the
 * larger of constants and ranges, every track raw, padding; 0 for a track type that is no scalar type. The workspace holds what the
 * launches of one call hand to each other (64 bytes per instance and 56 per instance and track, rounded up to 16); its contents before
 * and after a call mean nothing. */
uint64_t aclhip_scalar_compress_bound(uint32_t track_type, uint32_t num_tracks, uint32_t num_samples);
uint64_t aclhip_scalar_compress_workspace_bytes(uint32_t num_instances, uint32_t max_tracks);

/* The definition. All arithmetic is fp32, one IEEE operation at a time, never fused, denormals kept. The array has T tracks of C floats
 * and S samples; track b has precision p_b = track_precisions[b], or desc->precision. v[s][b][c] is a sample value; num_bits(r) is r for
 * rates 1 .. 23 and 32 for rate 24.
 *   1. Finite check. If any of the S * T * C floats is not finite, the status is ACLHIP_COMPRESS_NOT_FINITE.
 *   2. Looping (optimize_looping.scalar.h). With ACLHIP_COMPRESS_OPTIMIZE_LOOPS, an array registered with ACLHIP_LOOP_CLAMP and S > 1: if
 *      fabs(v[0][b][c] - v[S-1][b][c]) <= p_b for EVERY track and component, S becomes S - 1 and the blob is wrap optimized -- the whole
 *      list or nothing. An array registered with ACLHIP_LOOP_WRAP keeps S and is wrap optimized without a vote, with or without the
 *      flag. Everything below uses the new S.
 *   3. Ranges (track_range_impl.h:44-63), per track and component: min starts at 1e10F, max at -1e10F; in ascending sample order
 *      min = (min < x) ? min : x and max = (max > x) ? max : x (SSE minps / maxps: the second operand wins a tie); extent = max - min.
 *      The start values take part: a track whose samples all lie above 1e10 has min = 1e10. When the extreme is a zero, its sign is that
 *      of the LAST sample equal to it (+0 and -0 compare equal) -- min and extent are written into the blob, so this shows in the bytes.
 *      The kernel's parallel reduction gives those bits.
 *   4. Constant tracks: track b is constant iff fabs(extent[c]) < p_b for every component, strictly: with p_b == 0 nothing is constant,
 *      and a flat track ends at bit rate 1.
 *   5. Normalization (normalize.scalar.h:44-76) of the other tracks: n = (x - min) / extent, the division correctly rounded;
 *      n = (n < 1) ? n : 1; n = 0 where extent < 0.000000001F.
 *   6. Bit rate (quantize.scalar.h:84-160): best starts at 24 (raw); the rates r = 23, 22, ..., 1 are tried in that order.
 *      max_value = float((1u << r) - 1), inv = 1.0F / max_value, q = floorf(n * max_value + 0.5F) (round_symmetric of a value >= 0),
 *      d = (q * inv) * extent + min as a multiply, a multiply and an add; rate r passes iff fabs(x - d) <= p_b for every sample and
 *      component. The first rate that fails ends the search, even if a lower one would pass again; best is the last rate that passed.
 *   7. The blob (compress.scalar.impl.h:93-251, write_track_data_impl.h): raw_buffer_header { size, hash }; tracks_header { the
 *      compressed_tracks tag, version 10 (latest), uniformly_sampled, the track type, T, S, the sample rate, bit 30 of the packed word
 *      when wrap optimized, no metadata }; scalar_tracks_header { num_bits_per_frame, and the offsets of the four sections from its own
 *      start }. The sections in order: one byte per track -- 0 for a constant track, best otherwise --, padded to 4 bytes; C floats of
 *      sample 0 per constant track; C floats of min, then C of extent, per track of rate 1 .. 23; ONE bit stream, most significant bit
 *      first: per sample ascending, per track ascending with the constant ones skipped, per component ascending, num_bits(best) bits --
 *      uint32(q) for rates 1 .. 23, the float's own 32 bits for rate 24 --, padded to a whole byte (num_bits_per_frame is the bits of one
 *      sample); 15 zero bytes. size is the total, hash is FNV-1a 32 (core/hash.h) over [8, size).
 *   A NaN in track_precisions makes nothing constant and every rate fail: the track stays raw. Values of track_precisions are not checked.
 *   Refused per instance (ACLHIP_COMPRESS_REFUSED, counted, decided in front of any write to the row): an unknown or retired handle (0
 * included); T > max_tracks; track_precisions with T > num_track_precisions; a blob larger than blob_stride_bytes -- known after the
 * analysis and before the write, so a stride that is too small never writes outside its row; a bit stream of 2^32 bits or more (the
 * reference counts them in 32 bits).
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): raws, desc, blobs,
 * results or desc->workspace == NULL; blobs, the stride or the workspace not 16 byte aligned; a stride of 0; results not 8 byte aligned;
 * unknown flags or reserved fields that are not 0; a precision that is negative or not finite; track_precisions with a count of 0;
 * max_tracks == 0; the blob rows, the results or the workspace overlapping one another, raws or track_precisions.
 *   The call is stream ordered, uploads nothing and can be captured into a graph. Five launches (DESIGN.md 4.7 "Scalar compression"):
 * the vote per instance; the analysis, one wave per (instance, track); the layout, one wave per instance, which also stores headers,
 * metadata, constants and ranges; the bit stream, one lane per output dword gathering the values that fall into it (no atomics: the
 * same bytes on every run); the hash, serial in the bytes of a blob, one wave per blob with the chain on the scalar unit.
 *   Left out (nothing here precludes them): the variable bit rates of the transform (qvvf) compressor (its raw formats exist:
 * aclhip_compress_raw_tracks_batch, below); the optional metadata sections (names, descriptions) for scalar lists;
 * output_index remapping and stripped tracks; registering a clip straight from a device blob (aclhip_register_clip takes a host
 * pointer: runtime.compress_scalar_tracks copies back); the C++ mirror in aclhip.hpp; instance lists.
 *   What it costs (no time is promised; one MI355X, 4 096 instances over 256 distinct float1f arrays of 256 tracks x 120 samples -- the
 * bench's scalar list shape -- at precision 1e-4, where the rates spread from constant to 17; medians of three interleaved rounds of 20
 * launches; tools/scalar_compress.py, profiles/scalar_compress.md, DESIGN.md 4.7 "Scalar compression"): 3.57 ms a batch, 0.87 us an
 * array, next to the reference's compress_track_list over the same instances on the same box: 27.97 s on one thread, 1.83 s on 16.
 * By phase: vote 3.8 us, analysis 1 508 us (42 %), layout 54 us, bit stream 946 us (26 %), hash 1 061 us (30 %). The hash is a serial
 * chain per blob: for ONE large array it is the call's critical path, and nothing was built against that. */
aclhip_status aclhip_compress_raw_scalar_tracks_batch(aclhip_context* context,
	const aclhip_raw_scalar_tracks* raws /* DEVICE [num_instances] */, uint32_t num_instances,
	const aclhip_scalar_compress_desc* desc, void* blobs /* DEVICE */, uint64_t blob_stride_bytes,
	aclhip_compress_result* results /* DEVICE [num_instances] */, void* stream);

/* ---- compress_track_list for raw track arrays, raw formats ---------------------------------------------------------------------------------
 * acl::compress_track_list for a track_array_qvvf with the reference's RAW compression settings -- rotation_format = quatf_full,
 * translation_format = scale_format = vector3f_full: get_raw_compression_settings() (compression/impl/compress.transform.impl.h:138-530
 * and the files it calls) --, batched: a registered raw track array becomes a LOSSLESS `compressed_tracks` blob where it lives, one that
 * every consumer of this library takes. With these settings the reference segments nothing, reduces no range, takes no looping vote,
 * tests constant and default sub-tracks binary and stores every animated sample as its own 32 bit words; what remains is the transform
 * blob writer. THE BLOB IS BYTE FOR BYTE THE REFERENCE'S for the same samples and settings, hash included; the tests hold every byte.
 *   Instance i compresses array raws[i] into (char*)blobs + i * blob_stride_bytes; blobs and the stride are 16 byte aligned. The launch
 * writes every byte of [0, size) itself -- padding and the 15 trailing zero bytes included -- and touches nothing behind `size`. Handles
 * may repeat; arrays of different shapes share a launch. results[i] = { status, size } says how it went (aclhip_compress_result). */
#define ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES 2u   /* compression_settings::metadata.include_parent_track_indices */
#define ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS 4u     /* ...include_track_descriptions; implies the parent indices, as in the reference */
#define ACLHIP_COMPRESS_NOT_NORMALIZED 3u                 /* aclhip_compress_result::status: a rotation fails rtm::quat_is_normalized: size 0, row untouched */

typedef struct aclhip_transform_compress_desc
{
	uint32_t flags;                        /*  0  ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES, ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS;
	                                              ACLHIP_COMPRESS_OPTIMIZE_LOOPS is accepted and changes nothing (the reference's rule for raw settings) */
	uint32_t max_tracks;                   /*  4  tracks the workspace was sized for; an instance with more is refused */
	const void* default_pose;              /*  8  DEVICE or NULL: QVV48 record b = track_desc_transformf::default_value of track b, shared by the
	                                              launch, 16 byte aligned; NULL = identity / zero / one */
	const uint32_t* parent_indices;        /* 16  DEVICE or NULL (every track a root): desc.parent_index, ACLHIP_NO_PARENT for a root; metadata only */
	const float* track_precisions;         /* 24  DEVICE or NULL (-> precision): metadata only */
	const float* track_shell_distances;    /* 32  DEVICE or NULL (-> shell_distance): metadata only */
	uint32_t num_table_tracks;             /* 40  entries of every non-NULL table above */
	float precision;                       /* 44  reference default 0.0001F */
	float shell_distance;                  /* 48  reference default 1.0F; 4 bytes of padding follow */
	void* workspace;                       /* 56  DEVICE, 16 byte aligned, aclhip_transform_compress_workspace_bytes(num_instances, max_tracks) bytes */
	uint64_t reserved[2];                  /* 64  0 */
} aclhip_transform_compress_desc;          /* 80 bytes */

/* Host only. The bound of a blob: 100 + 12 * ceil(T / 16) + 40 * T * S + (with metadata: 4 * T, + 48 * T with descriptions, + 20; without:
 * 15), rounded up to 16 -- headers, sub-track types, every sub-track animated, metadata or the tail; computed 128 bits wide and capped at
 * the largest multiple of 16, so absurd counts do not wrap. The workspace holds what the launches of one call hand to each other (64
 * bytes per instance, 1 + 6 per instance and track, each part rounded up to 16); its contents before and after a call mean nothing. */
uint64_t aclhip_transform_compress_bound(uint32_t num_tracks, uint32_t num_samples, uint32_t flags);
uint64_t aclhip_transform_compress_workspace_bytes(uint32_t num_instances, uint32_t max_tracks);

/* The definition. The array has T tracks and S samples of QVV48 records; the USED LANES of a record are the four of the rotation and xyz
 * of translation and scale. The fourth lanes of translations and scales are never read, neither of the samples nor of default_pose. (The
 * reference compares all four lanes of its vector4f; a caller's array says nothing about the fourth. This call is the reference for track
 * arrays and default values whose fourth lanes agree, which is what rtm::vector_load3 and rtm::vector_set(x, y, z) make.)
 *   1. Checks over the registered samples. Every used lane must be finite, or the status is ACLHIP_COMPRESS_NOT_FINITE (the reference's
 *      "Some samples are not finite"). Every rotation must pass rtm::quat_is_normalized: fabs(((x * x + z * z) + (y * y + w * w)) - 1.0F)
 *      < 0.00001F, fp32, one IEEE operation at a time in this order (rtm::vector_dot), or the status is ACLHIP_COMPRESS_NOT_NORMALIZED:
 *      the reference renormalizes such a rotation (clip_context.impl.h:147-153) through rtm::quat_normalize, which starts from the x86
 *      reciprocal square root estimate -- not bit-reproducible between CPU vendors --, and this call promises bytes; it does
 *      not normalize some other way. NOT_FINITE wins when both hold: the reference tests finiteness on the value it would store.
 *   2. Looping. Nothing is removed (optimize_looping returns at once for raw settings). An array registered with ACLHIP_LOOP_WRAP keeps S
 *      and sets the header's wrap-optimized bit (clip_context.impl.h:87,103, compress.transform.impl.h:427).
 *   3. Per sub-track (compact.transform.h:213-346, track_stream.h:373-381): CONSTANT iff every sample compares equal (==, so -0 == +0) to
 *      sample 0 in every used lane; DEFAULT iff it is constant and sample 0 compares equal to the default value in every used lane. A
 *      default sub-track stores nothing; a constant one the bytes of sample 0, 16 for a rotation and 12 otherwise; the others are ANIMATED.
 *   4. has_scale is false iff every scale sub-track is default; then the scale third of the sub-track types and the scale data are absent.
 *   5. The blob (compress.transform.impl.h:287-530, write_segment_data.h, write_sub_track_types.h, write_stream_data.h): raw_buffer_header
 *      { size, hash }; tracks_header { the compressed_tracks tag, version 10 (latest), uniformly_sampled, qvvf, T, S, the sample rate, the
 *      packed word: has_scale, default scale 1, the three full formats, no database, no trivial default values (the reference asks
 *      quat_near_identity with a threshold of 0, which holds for no rotation), no stripped key frames, wrap optimized, has metadata };
 *      transform_tracks_header { one segment, no variable sub-tracks, the three animated and the three constant counts, no database, the
 *      offsets from its own start }; one segment_header { the bits of one animated pose, of its rotations, of its translations, the
 *      offset of the segment's data }; the sub-track types, 2 bits each (0 default, 1 constant, 2 animated), 16 per 32 bit word with the
 *      first track in the top bits, rotations, then translations, then scales, each type starting a new word; the constant data:
 *      rotations, translations, scales, each in track order; no range data and no per-track format data; the animated stream: per sample
 *      ascending the animated rotations xyzw, the translations xyz, the scales xyz, each in track order (output_index is the identity),
 *      every float as a 32 bit word, most significant byte first.
 *   6. Metadata (write_track_metadata.h:106-194), with either flag: T parent indices (parent_indices[b] when it is < T, else
 *      ACLHIP_NO_PARENT); with ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS 12 floats per track: precision, shell distance, the default
 *      rotation xyzw, translation xyz, scale xyz; the optional_metadata_header { no list name, no track names, the two offsets from the
 *      blob's start, no contributing error } ends the blob. Without metadata the blob ends in 15 zero bytes.
 *   7. size is the total, hash is FNV-1a 32 (core/hash.h) over [8, size).
 *   compression_settings::level, precision and shell_distance change no byte outside the descriptions.
 *   Refused per instance (ACLHIP_COMPRESS_REFUSED, counted by aclhip_get_rejected_instance_count, decided in front of any write to the
 * row): an unknown or retired handle (0 included); T > max_tracks; any table given and T > num_table_tracks; a blob larger than
 * blob_stride_bytes; an animated stream of 2^32 bits or more (the reference counts them in 32 bits).
 *   ACLHIP_ERROR_INVALID_ARGUMENT, decided before any device call, each with a message (with or without a context): raws, desc, blobs,
 * results or desc->workspace == NULL; blobs, the stride, the workspace or default_pose not 16 byte aligned; a stride of 0; results not 8
 * byte aligned; a table not 4 byte aligned; unknown flags or reserved fields that are not 0; a precision or a shell distance that is
 * negative or not finite; a table given with num_table_tracks == 0; max_tracks == 0; the blob rows, the results or the workspace
 * overlapping one another, raws or a table.
 *   The call is stream ordered, uploads nothing and can be captured into a graph. Four launches (DESIGN.md 4.7 "Transform compression
 * (raw formats)"): the analysis, one wave per (instance, track), which leaves one flag byte per track and uses no atomics; the layout,
 * one wave per instance, which decides the statuses and the refusal and stores headers, sub-track types, constants, metadata and the
 * tail; the stream, one lane per output dword (one 4 byte load, a byte swap, one coalesced store); the scalar compressor's hash.
 *   Left out (nothing here precludes them): the variable formats and everything they need (segmenting, range reduction, the bit rate
 * search; the error metric over the hierarchy and quatf_drop_w_full exist: aclhip_compress_tracks_batch, below; so do the variable formats at given
 * bit rates, with segmenting and range reduction: aclhip_compress_tracks_variable_batch, below; so does the search that finds those rates:
 * aclhip_find_bit_rates_batch, below); additive bases (they exist for the formats that decide by a metric:
 * aclhip_compress_tracks_additive_batch, below; a raw blob of an additive1 clip would need only the header's default-scale bit); track
 * and list names; output_index remapping and
 * stripped tracks; a flag that normalizes rotations within a tolerance; the C++ mirror in aclhip.hpp.
 *   What it costs (no time is promised; one MI355X, 4 096 instances over 256 distinct arrays of 100 tracks x 301 samples -- the bench's
 * pose shape, 91 % of the rotations, a third of the translations and a tenth of the scales animated: 5.92 GB of samples, 2.43 GB of
 * blobs --; medians of three interleaved rounds of 20 launches; tools/transform_compress.py, profiles/transform_compress.md, DESIGN.md 4.7
 * "Transform compression (raw formats)"): 22.8 ms a batch, 5.6 us an array, next to the reference's compress_track_list over the same
 * instances on the same box: 35.5 s on one thread, 2.36 s on 16. By phase: analysis 1 098 us (5 %), layout 8 us, stream 1 966 us (9 %),
 * hash 19 692 us (87 %): 594 KB of serial chain per blob. The hash is the call, and nothing was built against that. */
aclhip_status aclhip_compress_raw_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_transform_compress_desc* desc, void* blobs /* DEVICE */, uint64_t blob_stride_bytes,
	aclhip_compress_result* results /* DEVICE [num_instances] */, void* stream);

/* ---- compress_track_list for raw track arrays: drop-w rotations, the rigid shell -----------------------------------------------------------
 * acl::compress_track_list for a track_array_qvvf with rotation_format = quatf_drop_w_full, translation_format = scale_format =
 * vector3f_full (compression/impl/compress.transform.impl.h:138-530), batched. Once the rotation format is not quatf_full the reference
 * normalizes every rotation, computes the RIGID SHELL of every transform from the hierarchy, takes the looping vote with the error metric,
 * converts rotations to positive w, decides constant and default ROTATION sub-tracks by the error metric at the shell and writes 96 bit
 * rotations; with these three formats it does nothing else: no segmenting, no range reduction, no search. A locked joint whose rotation
 * jitters below the precision loses its sub-track entirely.
 *   rotation_format == 0 (quatf_full) runs aclhip_compress_raw_tracks_batch's four launches: the bytes, statuses and refusals are that
 * call's for the same arguments, ACLHIP_COMPRESS_NOT_NORMALIZED included. Everything below is rotation_format == 2.
 *   THE BLOB IS THE REFERENCE'S for the same samples and settings IN EVERY BYTE BUT THE ROTATION VALUE WORDS (and the hash over them):
 * the reference normalizes through rtm::quat_normalize, which starts from the x86 reciprocal square root ESTIMATE -- not reproducible
 * between CPU vendors --; this call normalizes with the correctly rounded 1 / sqrt, the project's standing definition. The
 * words differ by at most a few ulp (measured: 1.2e-7 absolute; the tests hold 1e-5). Every decision -- constant, default, the vote --
 * is the reference's wherever its error is not within rounding of its precision.
 *   Rows, results, statuses, refusal counting, alignment rules, overlap checks, stream ordering, "uploads nothing" and graph capture are
 * as for aclhip_compress_raw_tracks_batch. aclhip_transform_compress_bound(T, S, flags) STAYS THE BOUND: a drop-w blob has the raw blob's
 * sections with 12 bytes where that has 16 per rotation, and never more samples: it is never larger than the raw one. */
typedef struct aclhip_compress_tracks_desc
{
	uint32_t rotation_format;              /*  0  acl::rotation_format8: 0 quatf_full, 2 quatf_drop_w_full */
	uint32_t translation_format;           /*  4  acl::vector_format8: 0 vector3f_full */
	uint32_t scale_format;                 /*  8  0 vector3f_full */
	uint32_t flags;                        /* 12  ACLHIP_COMPRESS_OPTIMIZE_LOOPS | ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES | ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS */
	uint32_t max_tracks;                   /* 16  tracks the workspace was sized for; an instance with more is refused */
	uint32_t num_table_tracks;             /* 20  entries of every non-NULL table below */
	const void* default_pose;              /* 24  DEVICE or NULL, as in the raw call */
	const uint32_t* parent_indices;        /* 32  DEVICE or NULL (every track a root): the hierarchy the shell is made from, and metadata */
	const float* track_precisions;         /* 40  DEVICE or NULL (-> precision) */
	const float* track_shell_distances;    /* 48  DEVICE or NULL (-> shell_distance) */
	float precision;                       /* 56  reference default 0.0001F */
	float shell_distance;                  /* 60  reference default 1.0F */
	void* workspace;                       /* 64  DEVICE, 16 byte aligned, aclhip_compress_tracks_workspace_bytes(num_instances, max_tracks) bytes */
	void* shell_metadata;                  /* 72  DEVICE or NULL, 8 byte aligned: [num_instances][max_tracks] { float local_shell_distance, precision }: what step 2
	                                              computed, for b < T of every instance whose shell was computed: all but those that are not finite or
	                                              refused for their handle, their track count or by step 0 (rotation_format 2 only) */
	uint64_t reserved[2];                  /* 80  0 */
} aclhip_compress_tracks_desc;             /* 96 bytes */

/* Host only. The raw call's workspace and 8 bytes per instance and track (the shell), each part rounded up to 16, 128 bits wide and capped. */
uint64_t aclhip_compress_tracks_workspace_bytes(uint32_t num_instances, uint32_t max_tracks);

/* The definition for quatf_drop_w_full. All arithmetic is fp32, one IEEE operation at a time, never fused, denormals kept. The array has
 * T tracks and S samples. Used lanes and fourth lanes are as in the raw call.
 *   Per-track values. prec_b = track_precisions[b] or precision. dist_b = track_shell_distances[b] or shell_distance. parent_b =
 * parent_indices[b] if the table is given and the value is < T, else none.
 *   Helpers. shell_error(d, A, B) is qvvf_transform_error_metric::calculate_error with scale (transform_error_metrics.h:335-358), as
 * aclhip_measure_pose_error_batch states it: the three points (d,0,0), (0,d,0), (0,0,d) through rtm::qvv_mul_point3 of A and of B,
 * sqrtf(((dx * dx) + (dy * dy)) + (dz * dz)) of each difference, the greatest of the three with a > b ? a : b.
 *   0. Parent refusal. An instance with a parent_b in [b, T) is ACLHIP_COMPRESS_REFUSED and counted, before any write to the row. The
 *      reference orders transforms by (parent + 1, index) (clip_context.impl.h:62-79): children before parents in reverse only when every
 *      parent index is smaller than its child's. For any other numbering its shell is an artefact of that sort; this call does not imitate it.
 *   1. Normalize, then the finite check. n = q * (1.0F / sqrtf(((x * x + z * z) + (y * y + w * w)))) for EVERY rotation
 *      (clip_context.impl.h:150). Any used lane not finite after that gives ACLHIP_COMPRESS_NOT_FINITE; a zero quaternion ends there, as
 *      in the reference. ACLHIP_COMPRESS_NOT_NORMALIZED does not occur: (0, 0, 0, 2) is normalized and compresses. This is the one step
 *      where the bytes are this library's and not the reference's.
 *   2. Rigid shell (rigid_shell_utils.h:51-170), from ALL S samples of the normalized, not yet sign-converted array. Start with local_b =
 *      dist_b, sprec_b = prec_b. Visit the tracks in DESCENDING index order (with parent < child: the reference's reverse parent-first
 *      order, siblings included). For track b: d = local_b; stretch = the maximum over the samples and over the three points (d,0,0),
 *      (0,d,0), (0,0,d) of sqrtf((x * x + y * y) + z * z) of qvv_mul_point3(point, sample), started from 0.0F, with a > b ? a : b;
 *      psd_b = stretch, plus prec_b when d != dist_b; when parent_b exists and psd_b > local_parent: local_parent = psd_b, sprec_parent =
 *      sprec_b. The comparison is strict: of siblings with equal psd the highest index wins, and the parent's own distance wins a tie.
 *      An array whose shell arithmetic produces a NaN intermediate (finite samples whose products overflow) is outside the definition: it
 *      ends with a status and without a fault, and its bytes mean nothing.
 *      shell_metadata, when given, receives { local_b, sprec_b } for b < T.
 *   3. Looping (optimize_looping.transform.h:178-243). With ACLHIP_COMPRESS_OPTIMIZE_LOOPS, an array registered ACLHIP_LOOP_CLAMP and
 *      S > 1: when NOT shell_error(local_b, sample 0 of b, sample S-1 of b) > sprec_b for every track, S becomes S - 1 and the blob is
 *      wrap optimized. An array registered ACLHIP_LOOP_WRAP keeps S and is wrap optimized without a vote. Steps 4 to 6 use the new S.
 *   4. Positive w (convert_rotation.transform.h:93-96). All four lanes of a rotation are xored with the sign bit of its w; a w of -0
 *      flips too.
 *   5. Sub-tracks (compact.transform.h:72-254, :401-420). A rotation is CONSTANT iff no sample s has shell_error(local_b, {r_s, t_s, s_s},
 *      {r_0, t_s, s_s}) > sprec_b. It is DEFAULT iff it is constant and the same holds with the default rotation in place of r_0; the
 *      default rotation is used as given in default_pose, not normalized and not converted. A constant rotation stores x, y, z of r_0, 12
 *      bytes, SWIZZLED (write_stream_data.h:213-267): the constant rotations in track order in groups of four, a group as its four x,
 *      its four y, its four z; a last group of n < 4 as n x, n y, n z. Translations and scales are as in the raw call: binary == against sample 0 and the default, over the S of step 3.
 *      has_scale is as in the raw call.
 *   6. The blob. It is the raw call's blob with four differences: quatf_drop_w_full in the packed header word; 12 byte constant
 *      rotations, swizzled as step 5 says; three words per animated rotation in the stream (x, y, z); the segment header's bit counts follow from that. Metadata
 *      is unchanged: the descriptions carry prec_b and dist_b, not the shell's values. Tail, size and hash are as there.
 *   Refused per instance, besides step 0: as in the raw call. ACLHIP_ERROR_INVALID_ARGUMENT, each with a message: everything the raw call
 * refuses; shell_metadata not 8 byte aligned or overlapping anything else the call reads or writes; a format value that is no format of
 * the reference (rotation 1 or >= 4, vector >= 2); the reference's variable formats (rotation 3, vector 1), which are not built.
 *   Five launches (DESIGN.md 4.7 "Transform compression (drop-w rotations, rigid shell)"): the shell, one wave per instance, tracks in
 * descending order with samples across the lanes, which also takes the step 0 refusal, the finite test and the vote; the analysis, one wave
 * per (instance, track): two shell error ballots for the rotation, the raw call's for translation and scale; the raw call's layout and
 * stream with three words per rotation; the hash. No atomics besides the refusal counter: the same bytes on every run.
 *   Left out: the variable formats, segmenting, range reduction and the bit rate search (all exist since:
 * aclhip_compress_tracks_variable_batch and aclhip_find_bit_rates_batch, below; so does the matrix error metric:
 * aclhip_compress_tracks_metric_batch, below; so do additive bases: aclhip_compress_tracks_additive_batch, below); track and list names; output_index
 * remapping; the C++ mirror in aclhip.hpp. What it costs: profiles/compress_tracks.md. */
aclhip_status aclhip_compress_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_compress_tracks_desc* desc, void* blobs /* DEVICE */, uint64_t blob_stride_bytes,
	aclhip_compress_result* results /* DEVICE [num_instances] */, void* stream);

/* ---- compress_track_list for raw track arrays: the variable formats at given bit rates --------------------------------------------------
 * acl::compress_track_list for a track_array_qvvf with rotation_format = quatf_drop_w_variable, translation_format = scale_format =
 * vector3f_variable (compression/impl/compress.transform.impl.h:138-530), batched, with ONE THING TAKEN OUT: find_optimal_bit_rates
 * (quantize.transform.h:1174-1550). The bit rate of every (segment, animated sub-track) is an INPUT: a device table, or one rate per
 * kind. Everything else of the variable compressor is here: sub-track compaction of all three kinds under the error metric, clip range
 * reduction, segmenting, segment range reduction with the 8 bit fix-up, quantization and the segmented, bit packed blob -- the format
 * the fast decode paths read. Handed the rates the reference chose (its blob's format bytes), the call writes the reference's blob in
 * every byte that does not depend on a rotation's normalization (see aclhip_compress_tracks_batch: the words that do are within a few
 * ulp, the quantized rotation fields within one code). Alone it is a fixed-rate lossy compressor whose output a caller grades with
 * the raw clip error. The call is these three formats and nothing else; mixed full / variable settings are aclhip_compress_tracks_batch's
 * to refuse.
 *   Rows, results, the statuses ACLHIP_COMPRESS_OK, ACLHIP_COMPRESS_NOT_FINITE and ACLHIP_COMPRESS_REFUSED, refusal counting, alignment
 * and overlap rules, stream ordering, "uploads nothing" and graph capture are as for the two calls above. This is an addition to ABI
 * version 6: new names only, no existing struct or function changes. */
typedef struct aclhip_compress_variable_desc
{
	uint32_t flags;                        /*   0  ACLHIP_COMPRESS_OPTIMIZE_LOOPS | ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES | ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS */
	uint32_t max_tracks;                   /*   4  tracks the workspace was sized for; an instance with more is refused */
	uint32_t max_samples;                  /*   8  samples the workspace was sized for; an instance with more (behind the looping vote) is refused */
	uint32_t num_table_tracks;             /*  12  entries of every non-NULL per-track table below */
	const void* default_pose;              /*  16  DEVICE or NULL, as in the raw call */
	const uint32_t* parent_indices;        /*  24  DEVICE or NULL (every track a root) */
	const float* track_precisions;         /*  32  DEVICE or NULL (-> precision) */
	const float* track_shell_distances;    /*  40  DEVICE or NULL (-> shell_distance) */
	float precision;                       /*  48  reference default 0.0001F */
	float shell_distance;                  /*  52  reference default 1.0F */
	void* workspace;                       /*  56  DEVICE, 16 byte aligned, aclhip_compress_variable_workspace_bytes(num_instances, max_tracks, max_samples) bytes */
	void* shell_metadata;                  /*  64  DEVICE or NULL, 8 byte aligned: as in aclhip_compress_tracks_desc */
	const uint8_t* bit_rates;              /*  72  DEVICE or NULL, 4 byte aligned: the entry of (instance i, segment g, track b) is the 4 bytes { rotation, translation,
	                                               scale, 0 } at bit_rates + i * bit_rate_instance_stride + g * bit_rate_segment_stride + 4 * b. A table covers
	                                               aclhip_variable_compress_num_segments(S) rows of T entries for the S the array was REGISTERED with (the vote can
	                                               only lower the count). Entries of constant and default sub-tracks are not read; neither is the fourth byte. */
	uint64_t bit_rate_instance_stride;     /*  80  bytes, a multiple of 4; 0: every instance reads the same rows */
	uint64_t bit_rate_segment_stride;      /*  88  bytes, a multiple of 4; 0: every segment reads the same row */
	uint8_t rotation_bit_rate;             /*  96  with bit_rates == NULL: the rate of every animated rotation, */
	uint8_t translation_bit_rate;          /*  97  translation */
	uint8_t scale_bit_rate;                /*  98  and scale sub-track, in every segment */
	uint8_t reserved_rate;                 /*  99  0 */
	uint32_t reserved_word;                /* 100  0 */
	uint64_t reserved[2];                  /* 104  0 */
} aclhip_compress_variable_desc;           /* 120 bytes */

/* Host only. The segments of an array of num_samples samples: split_samples_per_segment (segment.transform.h:65-128) with the reference's
 * 16 ideal and 31 at most: one segment up to 31 samples; else ceil(S / 16) segments, the last one dealt out over the others when they
 * have room for it. Never larger for S - 1 than for S. */
uint32_t aclhip_variable_compress_num_segments(uint32_t num_samples);
/* Host only. An upper bound of a blob's size for ANY rate table, rounded up to 16: every sub-track animated at rate 24, with segment start
 * indices, segment headers, format bytes, padded segment range data and clip range data. 128 bits wide, capped like the other bounds. */
uint64_t aclhip_variable_compress_bound(uint32_t num_tracks, uint32_t num_samples, uint32_t flags);
/* Host only. aclhip_compress_tracks_workspace_bytes and, per instance, 72 bytes per track (the clip ranges), and per segment of
 * max_samples 32 bytes and 12 bytes per track (the prefix sums); each part rounded up to 16, 128 bits wide and capped. */
uint64_t aclhip_compress_variable_workspace_bytes(uint32_t num_instances, uint32_t max_tracks, uint32_t max_samples);

/* The definition. All arithmetic is fp32, one IEEE operation at a time, never fused, denormals kept; divisions are true divisions. The
 * array has T tracks and S samples. Steps 0 to 4 are those of aclhip_compress_tracks_batch, word for word: 0 parent refusal, 1 normalize
 * and the finite check, 2 the rigid shell { local_b, sprec_b } (shell_metadata receives it), 3 the looping vote (S may become S - 1),
 * 4 positive w. min(a, b) below is a < b ? a : b and max(a, b) is a > b ? a : b (rtm::vector_min, vector_max: of two that compare
 * equal, the second).
 *   5. Sub-tracks (compact.transform.h:72-346, 384-485). Per track, in the order rotation, translation, scale, each with shell_error at
 *      local_b against sprec_b over the S samples. Rotation: as in aclhip_compress_tracks_batch. Translation: CONSTANT iff no sample s has
 *      shell_error(local_b, {R_s, t_s, s_s}, {R_s, t_0, s_s}) > sprec_b, where R_s is the rotation AFTER ITS COMPACTION (the reference
 *      reads the stream it has already replaced): r_s of an animated rotation, r_0 of a constant one, the default rotation as given of a
 *      default one. DEFAULT iff constant and the same holds with the default translation in place of t_0. Scale: likewise with s_0 and the
 *      default scale, under the compacted rotation and the compacted translation (t_0 of a constant one, the default of a default one).
 *      has_scale is true throughout these tests (clip_context.impl.h:173) and afterwards "not every scale is default". Constant values are
 *      stored as in the drop-w call: rotations 12 bytes swizzled in fours, translations and scales x, y, z of sample 0.
 *   6. Clip ranges (normalize.transform.h:51-95, 200-262), per animated sub-track and component over the S samples of x, y, z (of the
 *      rotation as step 4 left it): lo = min(... min(min(1e10F, v_0), v_1) ..., v_S-1), hi likewise with max from -1e10F (a zero that is
 *      the minimum or maximum has the sign of the LAST sample that is a zero); extent = hi - lo. n_s = min((v_s - lo) / extent, 1.0F), or
 *      0.0F where extent < 0.000000001F.
 *   7. Segments: the sample counts of aclhip_variable_compress_num_segments' split, in order. One segment has no segment ranges.
 *   8. Segment ranges (only with more than one segment; normalize.transform.h:117-198). Per segment, animated sub-track and component:
 *      lo, hi of the n_s of the segment as in 6; fixup_range AS WRITTEN: q0 = clamp(floorf(lo * 255.0F), 0, 255), q1 = max(q0 - 1.0F, 0),
 *      pmin = q0 * (1.0F / 255.0F) where that is <= lo, else q1 * (1.0F / 255.0F); e0 = clamp(ceilf((hi - pmin) * 255.0F), 0, 255), e1 =
 *      min(e0 + 1.0F, 255), pext = e0 * (1.0F / 255.0F) where that is >= hi (the maximum, not the extent: the reference's comparison),
 *      else e1 * (1.0F / 255.0F). m_s = min((n_s - pmin) / pext, 1.0F), or 0.0F where pext < 0.000000001F. The stored bytes are
 *      pack(pmin, 8) and pack(pext, 8) per component, with pack(x, bits) = (uint32_t)floorf(x * (float)(2^bits - 1) + 0.5F)
 *      (math/scalar_packing.h:42-48: scalar_round_symmetric of a value that is not negative).
 *   9. Quantization (quantize.transform.h:370-660; pack_vector3_uXX_unsafe, _u48_, _u24_ of math/vector4_packing.h) at the entry's rate r
 *      (core/impl/variable_bit_rates.h:45): r in 1 .. 23 stores pack(m_s, r) per component (pack(n_s, r) with one segment), r bits each; 24
 *      stores the 32 bit words of the UNNORMALIZED x, y, z -- the rotation as step 4 left it, the translation or scale as registered --,
 *      96 bits; 0 ("constant in this segment") stores pack(n, 16) of the segment's FIRST sample, clip-normalized and not
 *      segment-normalized, in the sub-track's segment range bytes and nothing in the stream.
 *  10. The blob (compress.transform.impl.h:287-530, write_segment_data.h, write_range_data.h, write_stream_data.h:104-197, 312-531), every
 *      offset from the transform_tracks_header: the headers with quatf_drop_w_variable and vector3f_variable twice in the packed word,
 *      num_segments and num_animated_variable_sub_tracks (the animated rotations rounded up to 4, plus translations and scales); with more
 *      than one segment the segments' first samples and 0xFFFFFFFF; a 16 byte segment_header per segment (the bits of a pose, of its
 *      rotations, of its translations, the offset of the segment's data); sub-track types; constant data; CLIP RANGE DATA: rotations in
 *      groups of four as min xxxx yyyy zzzz then extent xxxx yyyy zzzz, a last group of n < 4 as rows of n; then translations, then
 *      scales, min.xyz extent.xyz each. Per segment, back to back: one FORMAT BYTE per animated sub-track, rotations (padded with zeros
 *      to a multiple of 4), translations, scales: the number of bits, 31 for rate 24; a zero byte up to an even offset; with more than one
 *      segment the SEGMENT RANGE DATA: rotations in groups of four, always padded to four with zeros, 24 bytes a group: min x of the
 *      four, min y, min z, extent x, y, z -- a rate 0 rotation's six rows hold x high byte, x low byte, y high, y low, z high, z low
 *      instead --; translations, then scales, six bytes each: min xyz extent xyz, or three little endian 16 bit words at rate 0; zero
 *      bytes up to a multiple of 4; the ANIMATED BIT STREAM: samples ascending, per sample the rotations, translations, scales in track
 *      order, three fields each, rate 0 sub-tracks absent, most significant bit first, continuous across samples, zero bits up to a whole
 *      byte once per segment. Then zero bytes up to a multiple of 4 and the metadata, or the 15 byte tail; size and hash as in the raw call.
 *   Refused per instance (ACLHIP_COMPRESS_REFUSED, counted, decided in front of any write to the row): everything the drop-w call
 * refuses; more samples behind step 3 than max_samples; an animated sub-track whose rate in a segment is above 24, or is 0 while the blob
 * has one segment (the reference allows 0 only where segment ranges exist, quantize.transform.h:1111-1140); a blob larger than the
 * stride or than 32 bits count, a segment of more than 2^32 bits. ACLHIP_ERROR_INVALID_ARGUMENT before any device call, each with a
 * message: everything aclhip_compress_tracks_batch refuses of the arguments both have; max_samples == 0; a rate table not 4 byte
 * aligned, a stride that is no multiple of 4, a table that overlaps the rows, the results, the workspace or the shell metadata (its
 * extent taken as (num_instances - 1) instance strides, (aclhip_variable_compress_num_segments(max_samples) - 1) segment strides and
 * 4 * max_tracks bytes); without a table a uniform rate above 24; reserved fields that are not 0.
 *   Six launches (DESIGN.md 4.7 "Transform compression (variable formats at given bit rates)"): the drop-w call's shell kernel; the
 * analysis, one wave per (instance, track): six shell error ballots in three passes and the clip ranges by butterfly; the layout, one wave
 * per instance: per segment the prefix sums of the bit widths in stream order into the workspace, the refusals, then everything but
 * segment ranges and streams; the segment ranges, one wave per (instance, segment) with lanes over the animated sub-tracks; the stream,
 * one lane per output dword, which finds its sub-track in the prefix sums and recomputes every component; the hash. No atomics besides
 * the refusal counter and no zero fill: the same bytes on every run.
 *   Left out: the bit rate search (a call of its own: aclhip_find_bit_rates_batch, below, writes the table this call reads); mixed full /
 * variable formats; keyframe stripping, database support and the
 * contributing error (the matrix error metric: aclhip_compress_tracks_variable_metric_batch, below; additive bases:
 * aclhip_compress_tracks_variable_additive_batch, below); track and list names; output_index remapping; the C++ mirror in
 * aclhip.hpp; anything against the serial hash. What it costs: profiles/compress_variable.md. */
aclhip_status aclhip_compress_tracks_variable_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_compress_variable_desc* desc, void* blobs /* DEVICE */, uint64_t blob_stride_bytes,
	aclhip_compress_result* results /* DEVICE [num_instances] */, void* stream);

/* ---- the variable formats' bit rate search ---------------------------------------------------------------------------------------------
 * acl::find_optimal_bit_rates (compression/impl/quantize.transform.h:1174-1523) for quatf_drop_w_variable / vector3f_variable /
 * vector3f_variable and the qvvf error metric at the compression levels lowest, low and medium, batched: THE RATE TABLE
 * aclhip_compress_tracks_variable_batch reads, in exactly that call's layout. "Search, then compress" with the same settings is the
 * reference's compress_track_list at those levels -- up to the one step where this library's bytes are its own, the normalization of
 * rotations (aclhip_compress_tracks_batch, step 1): a last bit there can flip a comparison that sits on a threshold, and the search
 * then takes another road. Measured against the reference on 28 clips (tests/test_bit_rate_search_oracle.py): 0.56 % of the animated
 * sub-track rates differ, 2.5 % in the worst clip, the stream bits by 0.11 % -- what the reference shows against itself when its input
 * rotations move by one ulp (0.51 %, 2.5 %, 0.10 %).
 *   Results (size 0), the statuses ACLHIP_COMPRESS_OK, ACLHIP_COMPRESS_NOT_FINITE and ACLHIP_COMPRESS_REFUSED, refusal counting,
 * alignment rules, stream ordering, "uploads nothing" and graph capture are as for aclhip_compress_tracks_variable_batch. This is an
 * addition to ABI version 6: new names only, no existing struct or function changes. */
typedef struct aclhip_find_bit_rates_desc
{
	uint32_t flags;                        /*   0  as aclhip_compress_variable_desc: ACLHIP_COMPRESS_OPTIMIZE_LOOPS decides the samples; the two INCLUDE flags are accepted */
	uint32_t max_tracks;                   /*   4  tracks the workspace was sized for; an instance with more is refused */
	uint32_t max_samples;                  /*   8  samples the workspace was sized for; an instance with more (behind the looping vote) is refused */
	uint32_t num_table_tracks;             /*  12  entries of every non-NULL per-track table below */
	const void* default_pose;              /*  16  DEVICE or NULL, as in the raw call */
	const uint32_t* parent_indices;        /*  24  DEVICE or NULL (every track a root) */
	const float* track_precisions;         /*  32  DEVICE or NULL (-> precision) */
	const float* track_shell_distances;    /*  40  DEVICE or NULL (-> shell_distance) */
	float precision;                       /*  48  reference default 0.0001F */
	float shell_distance;                  /*  52  reference default 1.0F */
	void* workspace;                       /*  56  DEVICE, 16 byte aligned, aclhip_find_bit_rates_workspace_bytes(num_instances, max_tracks, max_samples) bytes */
	void* shell_metadata;                  /*  64  DEVICE or NULL, 8 byte aligned: as in aclhip_compress_tracks_desc (the CLIP's shell of step 2, not S0's) */
	uint32_t level;                        /*  72  acl::compression_level8: 0 lowest, 1 low, 2 medium -- one search: the reference only branches at >= high */
	uint32_t reserved_word;                /*  76  0 */
	uint64_t reserved[2];                  /*  80  0 */
} aclhip_find_bit_rates_desc;              /* 96 bytes */

/* Host only. aclhip_compress_variable_workspace_bytes and, per instance and segment of max_samples, 16 bytes and 82 bytes per track (the
 * segment ranges as 18 floats, the segment's shell, an entry of the chain under work); each part rounded up to 16, 128 bits wide, capped. */
uint64_t aclhip_find_bit_rates_workspace_bytes(uint32_t num_instances, uint32_t max_tracks, uint32_t max_samples);

/* The definition. All arithmetic is fp32, one IEEE operation at a time, never fused, denormals kept; divisions are true divisions. Steps
 * 0 to 8 are those of aclhip_compress_tracks_variable_batch, word for word: the statuses, the samples S behind the vote, the sub-track
 * types, has_scale, the clip ranges {lo, extent}, the segments, and per segment and animated sub-track {pmin, pext} and m_s (n_s with
 * one segment). The search runs per segment; nothing of one segment enters another. normalize(q) is step 1's. A rotation made from
 * x, y, z is Q(x, y, z) = normalize((x, y, z, sqrtf(fabsf(((1.0F - x * x) - y * y) - z * z)))) (rotation_to_quat_32, rtm::quat_normalize).
 *   S0. THE SEGMENT'S SHELL (quantize.transform.h:232, rigid_shell_utils.h:175-283). The search does not use step 2's shell. For every
 *      segment the reference recomputes {local_b, sprec_b} by step 2's walk -- the same order, the same strict comparison, the same
 *      "+ prec_b when d != dist_b" -- over the segment's samples of WHAT THE SEGMENT'S STREAMS HOLD at that point of the compressor, not
 *      of the registered transforms: per kind the x, y, z of m_s of an animated sub-track (the range-normalized sample), of sample 0 of a
 *      constant one (the rotation as step 4 left it), of the default of a default one; the rotation is Q of its three. Both errors below
 *      use this {local_b, sprec_b}. (With the clip's shell in their place 10.7 % of the reference's rates are missed instead of 0.56 %.)
 *   S1. The sample a rate stands for (sample_streams.h:163-212, 306-355, 446-495), a pure function of (sub-track, sample, rate): the
 *      reference's track_bit_rate_database is a cache of it and is not rebuilt. decay(x, bits) = floorf(x * (float)(2^bits - 1) + 0.5F) *
 *      (1.0F / (float)(2^bits - 1)) per component (decay_vector3_uXX, _u48). For an animated sub-track at rate r and sample s: r in
 *      1 .. 23: v = decay(m_s, r), then v * pext + pmin (only with more than one segment), then v * extent + lo, a multiply then an add
 *      each; r = 0: decay(n of the segment's FIRST sample, 16), then * extent + lo only; r = 24: the unnormalized x, y, z of step 9.
 *      A rotation is Q(v). A constant sub-track contributes its sample 0 (a rotation as normalize of what step 4 left), a default one
 *      the default as given. The S1 transform of a track at rates (r, t, s) is {rotation, translation, scale} so made.
 *   S2. The two errors (:674-867), both of track b at local_b against sprec_b of S0. E(A, B) is shell_error(local_b, A, B) when has_scale;
 *      otherwise calculate_error_no_scale: only the points (d,0,0) and (0,d,0), through qvv_mul_point3 WITHOUT the scale
 *      (transform_error_metrics.h:360-378). The raw transform of a sample is {normalize(r_s as step 4 left it), t_s, s_s}. LOCAL error:
 *      E(raw, S1 transform). OBJECT error: both sides multiplied down the chain root = c_0, c_1 .. c_n = b: O_0 = L_0, O_k =
 *      {normalize(quat_mul(L_k.q, O_k-1.q)), quat_mul_vector3(L_k.t * O_k-1.s, O_k-1.q) + O_k-1.t, L_k.s * O_k-1.s} with has_scale,
 *      without it the same with every scale 1 (qvv_normalize of qvv_mul / qvv_mul_no_scale, :289-333; always the quaternion route: a
 *      negative scale does not leave it); then E(O_n raw, O_n lossy). A scan UNTIL THE ERROR IS TOO HIGH returns the maximum, from 0.0F,
 *      over the samples up to and including the first whose error is >= sprec_b; a scan TO THE END the maximum over all.
 *   S3. Local phase (:869-989, 1111-1140), per track with an animated sub-track. The list: every tuple of one rate 0 .. 24 per animated
 *      kind (rotation, translation, scale in that order), sorted by the summed bits of a component (rate r: r bits, 24: 32), then by the
 *      rates themselves, the first kind first -- the rule of the reference's generator script; the library makes the three lists from it
 *      at compile time. With one segment a tuple with a rate of 0 is skipped. best_error = 1e10F; walk the list: the tuple's local error
 *      scanned until too high; error < best_error (strict) replaces best and best_error, across sizes. At the first tuple whose size
 *      differs from the one before it while best_error < sprec_b, stop. The track's rates are best; the byte of a sub-track that is not
 *      animated is 255 and never changes.
 *   S4. Object phase (:997-1098, 1227-1475). Tracks in the order (parent_b + 1 in 32 bits, b): roots first. Per track b with chain c_0 .. c_n
 *      and all scans until too high unless said: error = object error of b; if error < sprec_b the track is done. Else loop while
 *      error >= sprec_b: for k = n down to 0 (own track first, then toward the root): INCREASE c_k -- of the candidates "c_k's scale + 1"
 *      (only with has_scale), "translation + 1", "rotation + 1", in that order, each only where that rate is below 24 (the reference's
 *      three nested loops with their breaks, written out in the kernel), the one whose object error MEASURED AT c_k, not at b, is lowest
 *      and strictly below b's error before the loop's round; none: c_k is skipped -- then the object error of b with c_k so increased;
 *      strictly below the best of this round so far: it becomes the round's best, and if also < sprec_b no further k is tried. A round
 *      that found none ends the loop; otherwise the best is applied and, unless it is < sprec_b, the loop goes on from its error. Then the
 *      object error of b TO THE END is taken (as is every error from here on), and while it is >= sprec_b: for k = n down to 0, while
 *      the error is >= sprec_b: the smallest of c_k's three bytes (the first of equals; 255 counts as 255) -- if it is >= 24, c_k is
 *      maxed out, next k --, or the translation when rotation == translation < 24 and the scale byte is >= 24, is raised by one; the
 *      error is measured again; c_k keeps the rates of its lowest error so far (its own at the start included) and the error goes on from
 *      that; < sprec_b ends everything. When every c_k was maxed out the track is done. The reference's last pass (rates to the maximum)
 *      is for quatf_full rotations only: never here. Every loop ends: a round of the first loop that goes on raises a rate, and rates stop
 *      at 24; in the last pass every c_k ends below the threshold or maxed out, so its outer loop runs once (it may LOWER rates again:
 *      c_k keeps its best).
 *   Output. Four bytes { rotation, translation, scale, 0 } per (instance i, segment g, track b) at bit_rates + i * instance_stride + g *
 *      segment_stride + 4 * b, for b < T and the segments the instance has behind the vote; 255 for a constant or default sub-track.
 *      Other rows and entries are not touched. An instance that ends with another status than ACLHIP_COMPRESS_OK writes nothing to its rows.
 *   Refused per instance: everything aclhip_compress_tracks_variable_batch refuses that does not concern rates or rows.
 * ACLHIP_ERROR_INVALID_ARGUMENT before any device call, each with a message: what that call refuses of the arguments both have;
 * max_samples == 0; a level of 3 or 4 (high, highest: not built) or above; a NULL table, one not 4 byte aligned, strides that are no
 * multiples of 4, a segment_stride below 4 * max_tracks or an instance_stride below aclhip_variable_compress_num_segments(max_samples)
 * segment strides (the writers of two rows must not meet); a table -- it is WRITTEN -- that overlaps anything else the call reads or writes.
 *   Five launches (DESIGN.md 4.7 "Bit rate search"): the shell and the analysis of the variable call, unchanged; per (instance, segment)
 * the segment ranges and S0; per (instance, segment, track) S3 from a table of S1 in LDS, lanes over the tuples of a size; per (instance,
 * segment) S4 with lanes over the samples. No atomics besides the refusal counter and no zero fill: the same bytes on every run.
 *   Left out: the levels high and highest (chains with two and three increments: aclhip_find_bit_rates_level_batch, below; the matrix error metric:
 * aclhip_find_bit_rates_metric_batch, below; additive bases: aclhip_find_bit_rates_additive_batch, below); the
 * contributing error and keyframe stripping. What it costs: profiles/bit_rate_search.md. */
aclhip_status aclhip_find_bit_rates_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_find_bit_rates_desc* desc, uint8_t* bit_rates /* DEVICE */, uint64_t instance_stride,
	uint64_t segment_stride, aclhip_compress_result* results /* DEVICE [num_instances] */, void* stream);

/* ---- the transform compressors with the error metric as an argument ----------------------------------------------------------------------
 * aclhip_compress_tracks_batch, aclhip_compress_tracks_variable_batch and aclhip_find_bit_rates_batch with the error metric their
 * decisions are taken by as an argument, as aclhip_measure_pose_error_metric_batch is to aclhip_measure_pose_error_batch: `metric` is
 * an aclhip_error_metric. What a clip is compressed towards is then what aclhip_measure_pose_error_metric_batch measures of it: the
 * reference names its matrix metric for rigs with non-uniform scale, where a QVV product cannot hold the shear a scaled parent puts on
 * a rotated child. This is an addition to ABI version 6: new names only, no existing struct, function or message changes.
 *   ACLHIP_METRIC_QVVF is the call without the argument: one host path, the same kernels, the same bytes. The three entry points above
 * are these with ACLHIP_METRIC_QVVF.
 *   An unknown metric is ACLHIP_ERROR_INVALID_ARGUMENT with a message, before any device call and before any other argument is looked at.
 *   rotation_format == 0 (quatf_full, the raw call through aclhip_compress_tracks_metric_batch) uses no metric: any known one is
 * accepted and gives the raw call's bytes.
 *   Everything else is the base call's, word for word: the descs, every refusal, message, status, result and refusal count, the
 * alignment and overlap rules, the workspace (the *_workspace_bytes functions above serve both metrics: nothing new lies in it), the
 * shell metadata, stream ordering, "uploads nothing" and graph capture.
 *   The definition for ACLHIP_METRIC_QVVF_MATRIX3X4F follows the reference's CODE (qvvf_matrix3x4f_transform_error_metric,
 * transform_error_metrics.h:389-462; the comment above that class says the local error stays in qvvf, the code converts wherever
 * needs_conversion(has_scale) holds). M(t) is step 1 of aclhip_pose_matrices_batch (rtm::matrix_from_qvv) of the transform t;
 * E_m(d, A, B) is step 3 of aclhip_measure_pose_error_metric_batch under this metric for two matrices: the points (d,0,0), (0,d,0), (0,0,d)
 * through point(p, T) of both, the largest of the three distances. In the definitions above, and in nothing else of them:
 *   Step 3, the looping vote (optimize_looping.transform.h:115-173): a track votes against the wrap iff
 *      E_m(local_b, M(first sample), M(last sample)) > sprec_b. Always the matrix route: has_scale is true at that point
 *      (clip_context.impl.h:173).
 *   Step 5, the compaction of constant and default sub-tracks (compact.transform.h:72-211): every shell_error(d, raw, lossy) is
 *      E_m(d, M(raw), M(lossy)), for the same reason always. In the drop-w call that is the rotation; in the variable call and the
 *      search all three kinds, each kind seeing the kinds before it as compacted, as there.
 *   S2 WITH has_scale (quantize.transform.h:223-314, 674-867). LOCAL error: E_m(local_b, M(raw), M(S1 transform)). OBJECT error: both
 *      sides go down the chain as matrices, O_0 = M(L_0), O_k = matrix_mul(M(L_k), O_k-1) -- step 2 of aclhip_pose_matrices_batch: the
 *      product is lhs first; nothing is normalized anywhere and a negative scale is no special case, a matrix needs none -- then
 *      E_m(local_b, O_n raw, O_n lossy). The two scans and their thresholds are unchanged.
 *   S2 WITHOUT has_scale: exactly ACLHIP_METRIC_QVVF's. The matrix metric inherits calculate_error_no_scale, qvv_mul_no_scale and
 *      qvv_normalize: a clip whose scales are all default gets the table of the qvvf search, byte for byte, wherever vote and
 *      compaction fell the same way.
 *   Unchanged: step 1's normalization; the clip's rigid shell of step 2 and S0's shell per segment (rigid_shell_utils.h never asks the
 *      metric: both stay qvv_mul_point3); ranges, the fix-up, quantization and S1; the permutation lists; every loop, order and strict
 *      comparison of S3 and S4; the blob's layout and the hash.
 *   Measured against the reference under its matrix metric on the 28 clips of tests/test_bit_rate_search_oracle.py
 * (tests/test_matrix_metric_compress_oracle.py): 0.25 % of the animated sub-track rates differ, 2.5 % in the worst clip, the stream bits
 * by 0.10 % -- the reference against itself with its input rotations one ulp away: 0.71 %, 3.6 %, 0.16 %. The two metrics differ from
 * each other in 12 % of those rates.
 *   The launches are the base calls' (DESIGN.md 4.7 "Transform compression (the matrix error metric)"): the metric is a template
 * argument of the five kernels that decide by it -- the shell kernel's vote, both analyses, the local and the object phase of the
 * search --, and the qvvf instantiations are the kernels as they were. The object phase carries two 3x4 matrices down the chain per lane
 * in the place of two QVVs; the local phase keeps its LDS image in QVV and applies M() behind the read.
 *   Left out: what the base calls leave out, but for the metric. What it costs: profiles/compress_metric.md. */
aclhip_status aclhip_compress_tracks_metric_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_compress_tracks_desc* desc, void* blobs /* DEVICE */, uint64_t blob_stride_bytes,
	aclhip_compress_result* results /* DEVICE [num_instances] */, uint32_t metric, void* stream);
aclhip_status aclhip_compress_tracks_variable_metric_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_compress_variable_desc* desc, void* blobs /* DEVICE */, uint64_t blob_stride_bytes,
	aclhip_compress_result* results /* DEVICE [num_instances] */, uint32_t metric, void* stream);
aclhip_status aclhip_find_bit_rates_metric_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_find_bit_rates_desc* desc, uint8_t* bit_rates /* DEVICE */, uint64_t instance_stride,
	uint64_t segment_stride, aclhip_compress_result* results /* DEVICE [num_instances] */, uint32_t metric, void* stream);

/* ---- the bit rate search at every compression level ----------------------------------------------------------------------------------------
 * aclhip_find_bit_rates_metric_batch with the levels it leaves out: `desc->level` is 0 to 4 (lowest, low, medium, high, highest) or
 * ACLHIP_LEVEL_AUTOMATIC, the level of acl::get_default_compression_settings(). With it "search, then compress" is the reference's
 * default compress_track_list. This is an addition to ABI version 6: new names only, no existing struct, function or message changes.
 *   Everything is that call's, word for word -- the desc, the table's layout, every check, refusal and status, the alignment and overlap
 * rules, the metric, stream ordering, "uploads nothing" and graph capture -- but for: the messages name this call ("bit rate level
 * search"); any other level is ACLHIP_ERROR_INVALID_ARGUMENT with a message that names the accepted ones; the workspace is
 * aclhip_find_bit_rates_level_workspace_bytes; and the second word of an instance's result (`size`, 0 from the other two calls) is THE
 * LEVEL THAT WAS SEARCHED, 0 to 4, for an instance that ends ACLHIP_COMPRESS_OK and 0 for any other.
 *   The levels 0, 1 and 2 give aclhip_find_bit_rates_metric_batch's table, byte for byte.
 *   AUTOMATIC (find_best_compression_level, compress.transform.impl.h:114-136) is decided per instance on the device, so a launch may
 * mix rigs: medium when the array has more than 500 samples AS REGISTERED (the reference resolves the level before its looping vote
 * removes a sample); otherwise by the longest chain of the instance, counted in bones from a root to a leaf over its tracks and
 * `parent_indices`: below 18 highest, below 25 high, else medium.
 *   HIGH AND HIGHEST change S4's first loop alone (quantize.transform.h:1250-1377); S0 to S3 and the last pass are as stated above. In
 * a round -- error >= sprec_b, original = best = error -- the reference calls calculate_bone_permutation_error once per SHAPE of
 * increments over the chain c_0 .. c_n, in this order: {1} (every level: the loop stated above); from high on {2} and, when n >= 1,
 * {1,1}; at highest also {3}, when n >= 1 {2,1}, and when n >= 2 {1,1,1}. A shape's ARRANGEMENTS put its increments on distinct links,
 * 0 elsewhere, and come in std::next_permutation order over the array of increments indexed by link, root first (the own track's
 * place changes fastest), from the arrangement with the increments on the last links in the order written: every shape starts at
 * its smallest arrangement and visits all, except {2,1}, which starts at "c_n-1 + 2, c_n + 1" and runs from there to the end, so
 * "c_n-1 + 1, c_n + 2" is never tried and a chain of two links tries one arrangement. For an arrangement, every link c_k with an
 * increment m is INCREASED by m: of the (rotation, translation, scale) increments that sum to m -- three nested loops 0 .. m, the
 * scale's 0 .. 0 without has_scale, each clamped at 24, a rate of 255 left alone, with the reference's rules at 24 (:1005-1046: behind
 * a rotation, translation or scale that reached 24 the loop of that kind ends; a sum other than m is passed over) -- the one whose
 * object error measured AT c_k is lowest and strictly below `original`, else c_k's rates as they are. An arrangement none of whose
 * links changed is skipped unmeasured. Otherwise the object error of b with those links so increased is taken: strictly below the
 * call's best so far (from `original`) it becomes the call's best, and if also < sprec_b the call ends at once. After a call: its
 * best strictly below the round's best replaces it, with its rates, and if < sprec_b the round and the loop end. A round none of
 * whose calls improved ends the loop; otherwise the best is applied and the loop goes on from its error. Every loop ends: a shape's
 * arrangements are finitely many, and a round that goes on has raised a rate, and rates stop at 24.
 *   Measured against the reference (tests/test_bit_rate_search_levels_oracle.py, which states the figures and the caps): the
 * differences are what the reference shows against itself with its input rotations one ulp away.
 *   Six launches (DESIGN.md 4.7 "Bit rate search", the levels): the five of aclhip_find_bit_rates_batch with one small launch in front of the
 * object phase that leaves the level per instance, and the object phase's second instantiation, which tries the wider shapes. What
 * INCREASING c_k by m gives does not change within a round: that kernel computes it once per round and link, where the reference
 * recomputes it for every arrangement, and keeps it in the workspace; no decision differs. What it costs: profiles/bit_rate_search_levels.md. */
#define ACLHIP_LEVEL_AUTOMATIC 100u        /* acl::compression_level8::automatic */

/* Host only. aclhip_find_bit_rates_workspace_bytes and, per instance, segment of max_samples and track, 12 bytes more (what
 * increasing a link of the chain under work by 1, 2 and 3 gives in this round); rounded up to 16, 128 bits wide, capped. */
uint64_t aclhip_find_bit_rates_level_workspace_bytes(uint32_t num_instances, uint32_t max_tracks, uint32_t max_samples);

aclhip_status aclhip_find_bit_rates_level_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_find_bit_rates_desc* desc, uint8_t* bit_rates /* DEVICE */, uint64_t instance_stride,
	uint64_t segment_stride, aclhip_compress_result* results /* DEVICE [num_instances] */, uint32_t metric, void* stream);

/* ---- the transform compressors for additive clips: compressed against their base -------------------------------------------------------------
 * aclhip_compress_tracks_batch, aclhip_compress_tracks_variable_batch and aclhip_find_bit_rates_level_batch with the one input of the
 * reference's call they leave out: compress_track_list(allocator, track_list, settings, additive_base_track_list, additive_format, ...)
 * (compression/impl/compress.impl.h:68-88). Every decision the reference takes for an additive clip is measured AFTER the clip has been
 * applied onto its base -- the rigid shell, the looping vote, constant and default compaction, the per-segment shell and both errors of
 * the search --, and for additive1 the header says default scale 0. Without the base a `relative` clip's rotation error is not levered
 * by the base's translation and an additive1 scale of 0.001 is not "1.001 times the base": the search spends its bits in the wrong
 * places. What a clip is compressed towards is then what runtime.raw_clip_error(additive_base=, additive_format=) measures of it.
 * This is an addition to ABI version 6: new names only; no existing struct, function, message or byte of an existing call changes.
 *   The metric is the reference's additive_qvvf_transform_error_metric<format> (transform_error_metrics.h:469-524): the qvvf metric
 * with apply_additive_to_base / apply_additive_to_base_no_scale in front. The reference has no additive matrix metric (the base class
 * asserts "Not implemented"): these calls take no metric argument. The search call is the level search: desc->level is 0 to 4 or
 * ACLHIP_LEVEL_AUTOMATIC, and the second result word is the level searched.
 *   With additive_format == ACLHIP_ADDITIVE_NONE the calls give exactly the base calls' results by the same kernels -- the base calls
 * being the three named above, the search with ACLHIP_METRIC_QVVF --, whatever base_raws is, NULL included. All six are fronts of one
 * host path.
 *   Everything not stated here is the base call's, word for word: the descs, refusals, statuses, alignment and overlap rules, stream
 * ordering, "uploads nothing", graph capture and the workspace: the existing *_workspace_bytes functions serve these calls. Nothing
 * of the base is stored: a base sample is read and normalized where it is used, and the normalization is a pure function of the sample.
 *   ACLHIP_ERROR_INVALID_ARGUMENT with a message, before any device call: a NULL aclhip_additive_base; an unknown format; reserved
 * fields that are not 0; a format other than NONE with base_raws NULL, or not 4 byte aligned; base_raws (num_instances handles)
 * overlapping anything the call writes; rotation_format == 0 (quatf_full) with a format other than NONE: the raw settings decide
 * nothing by a metric.
 *   ACLHIP_COMPRESS_REFUSED per instance, counted, before any write to its row: a base handle that is no live raw track array; a base
 * with fewer tracks than the instance (the reference would read out of bounds). ACLHIP_COMPRESS_NOT_FINITE: a base with a used lane
 * (rotation x, y, z, w as normalized; translation and scale x, y, z) not finite in any of ITS tracks and samples -- the reference's
 * "Some base samples are not finite". A base may have any sample count and any sample rate of its own.
 *   The definition, as the changes to steps 1 to 5 and 10 of aclhip_compress_tracks_batch / _variable_batch and to S0 to S4 of the search;
 * nothing else of them changes.
 *   base(b, s), the base's sample of track b that goes with sample s of the instance. Its rotation is normalize() of step 1
 *      (clip_context.impl.h:150: the base goes through the same initialize_clip_context; it is NOT made of positive w: no
 *      convert_rotation_streams runs over the base), translation and scale as registered. With S_b the base's sample count, rate_b its
 *      rate and D, D_b the two arrays' finite durations as registered: S_b == 1: key 0. Else t = s / rate; t = t < D ? t : D
 *      (rtm::scalar_min); x = ((t / D) * D_b) * rate_b; key0 = (uint32)x (never above S_b - 1 inside the definition; the kernels take
 *      S_b - 1 then), key1 = min(key0 + 1, S_b - 1); key = floorf((x - (float)key0) + 0.5F) == 0.0F ? key0 : key1
 *      (get_uniform_sample_key: find_linear_interpolation_samples_with_sample_rate with sample_rounding_policy::nearest, never looping,
 *      over the base's own count and rate; sample_streams.h:557-601, interpolation_utils.impl.h:143-201). In segments s is the index in
 *      the clip. The base is never interpolated. An instance of ONE sample has D = 0 and x is 0 / 0: the reference converts that NaN
 *      to an integer, which C++ leaves undefined; its x86 build gets key0 = 0 and an alpha that fails `== 0`: key = min(1, S_b - 1),
 *      which is what this library states and does.
 *   A(x) = apply_additive_to_base(format, base(b, s), x) (core/additive_utils.h:128-162): RELATIVE qvv_mul(x, base), always its
 *      quaternion route as everywhere else in the compressors: {quat_mul(x.q, base.q), quat_mul_vector3(x.t * base.s, base.q) + base.t,
 *      x.s * base.s}; ADDITIVE0 {quat_mul(x.q, base.q), x.t + base.t, x.s * base.s}; ADDITIVE1 the same with (1.0F + x.s) * base.s.
 *      Where the definition uses the _no_scale arithmetic (S2 without has_scale) it is apply_additive_to_base_no_scale (:145-174):
 *      RELATIVE {quat_mul(x.q, base.q), quat_mul_vector3(x.t, base.q) + base.t, 1}, the other two {quat_mul(x.q, base.q), x.t + base.t, 1}.
 *   Step 2, the clip's shell (rigid_shell_utils.h:93-138): the stretch is taken over A(sample) in the place of the sample. The finite
 *      test of step 1 is of the instance's own samples, as before, and of the base's.
 *   Step 3, the vote (optimize_looping.transform.h:115-173): shell_error(local_b, A_first(first), A_last(last)), where A_first applies
 *      onto the base's sample 0 and A_last onto the base's LAST sample, S_b - 1: they are not base(b, s).
 *   Step 5, compaction (compact.transform.h:124-207): both sides of every shell_error go through A with the same base(b, s), s the
 *      sample under test.
 *   Step 10, the header: the default-scale bit of the packed word is 0 under ADDITIVE1 and 1 otherwise (compress.transform.impl.h:422-423);
 *      has_trivial_default_values stays false. A caller whose additive1 clip rests at scale 0 says so in default_pose.
 *   S0, the segment's shell (rigid_shell_utils.h:212-246): the stretch over A(what the segment's streams hold), s the index in the clip.
 *   S2, the search's errors (quantize.transform.h:269-313, 720-762, 834-842): the raw side is A(raw) per track, before the walk down the
 *      chain; the lossy side is A(S1 transform); in the local and in the object error alike. The base here comes out of sample_streams
 *      (sample_streams.h:649-673): base(b, s) at the same key, its rotation normalized ONCE MORE -- rtm::quat_normalize of the already
 *      normalized value --, as written there. (Confirmed against the reference: the base's clip context is never compacted, so its
 *      three kinds are always read as animated and its has_scale is true: its scale is the registered one, never a default.)
 *   Unchanged: every loop, order, threshold and strict comparison of S3 and S4, the permutation lists, the levels, the ranges, the
 *      quantization and the layout.
 *   The launches are the base calls' (DESIGN.md 4.7 "Transform compression (additive bases)"): the base is a template argument of the
 *   seven kernels it enters -- the shell kernel, both analyses, the segment kernel, the local phase and the two instantiations of the
 *   object phase --, the format a word of the launch record; the instantiations without it serve NONE and every other call. The layout
 *   kernels take the header bit from their launch record.
 *   Left out: a base under quatf_full (an additive1 raw blob would need only the header bit); an additive matrix metric (the reference
 *   has none); the levels-free search with a base (levels 0 to 2 of this call are it); what the base calls leave out. Measured against
 *   the reference and what it costs: profiles/compress_additive.md. */
typedef struct aclhip_additive_base
{
	const aclhip_raw_tracks* base_raws;  /*   0  DEVICE [num_instances]: the base of instance i, a registered raw track array; NULL only with NONE */
	uint32_t additive_format;            /*   8  aclhip_additive_format: NONE, RELATIVE, ADDITIVE0, ADDITIVE1 */
	uint32_t reserved_word;              /*  12  0 */
	uint64_t reserved[2];                /*  16  0 */
} aclhip_additive_base;                  /* 32 bytes */

aclhip_status aclhip_compress_tracks_additive_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_compress_tracks_desc* desc, void* blobs /* DEVICE */, uint64_t blob_stride_bytes,
	aclhip_compress_result* results /* DEVICE [num_instances] */, const aclhip_additive_base* additive_base, void* stream);
aclhip_status aclhip_compress_tracks_variable_additive_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_compress_variable_desc* desc, void* blobs /* DEVICE */, uint64_t blob_stride_bytes,
	aclhip_compress_result* results /* DEVICE [num_instances] */, const aclhip_additive_base* additive_base, void* stream);
aclhip_status aclhip_find_bit_rates_additive_batch(aclhip_context* context, const aclhip_raw_tracks* raws /* DEVICE [num_instances] */,
	uint32_t num_instances, const aclhip_find_bit_rates_desc* desc, uint8_t* bit_rates /* DEVICE */, uint64_t instance_stride,
	uint64_t segment_stride, aclhip_compress_result* results /* DEVICE [num_instances] */, const aclhip_additive_base* additive_base, void* stream);

/* ---- multi-GPU ---------------------------------------------------------------------------------- */

/* Decoding never needs a collective: every GPU decodes its own contiguous shard of the instance list. Only a
 * caller that wants every rank to see every pose gathers the shards afterwards: one RCCL all-gather over xGMI.
 * `rccl_comm` is the caller's ncclComm_t (one process per GPU); `shard_poses` are this rank's `shard_bytes` bytes, `all_poses`
 * receives world_size * shard_bytes bytes in rank order (in place when shard_poses == all_poses + rank * shard_bytes).
 * DEVICE pointers; asynchronous on `stream`. librccl.so.1 is loaded on first use: ACLHIP_ERROR_DEVICE when it is absent. */
aclhip_status aclhip_all_gather_poses(aclhip_context* context, void* rccl_comm, const void* shard_poses, void* all_poses, uint64_t shard_bytes, void* stream);

/* The RCCL aclhip_all_gather_poses would call, found the same way -- a ncclAllGather already visible in the process, else a library
 * already loaded under RCCL's soname, else a fresh load of librccl.so.1 / librccl.so (the communicator was made by the RCCL of the
 * caller's process: that one must run) -- and asked for its version, without a communicator. A check to run BEFORE a multi-GPU job:
 * out_version RCCL's version code (22606 = 2.26.6), out_path the file the entry point lives in, out_how how it was found (any of the
 * three may be NULL). ACLHIP_ERROR_DEVICE when RCCL or one of the two symbols is missing. No reference counterpart. */
aclhip_status aclhip_probe_rccl(int* out_version, char* out_path, uint32_t path_capacity, char* out_how, uint32_t how_capacity);

/* Peer gather: when ONE GPU wants every pose (the one that renders), each other GPU pushes its shard straight into that GPU's
 * buffer over its own xGMI link -- the destination's seven links work concurrently and no shard travels twice -- instead of a ring
 * collective that also gives every rank every shard. One process per GPU:
 *   destination:  aclhip_peer_export_buffer(ctx, all_poses, handle)     72 opaque bytes (a HIP IPC memory handle + offset), sent to the
 *                                                                      other processes by whatever they already talk over
 *   every source: aclhip_peer_open_buffer(ctx, handle, &peer)           maps the destination's buffer (once)
 *                 aclhip_push_poses_to_peer(ctx, peer, rank * shard_bytes, shard_poses, shard_bytes, stream)   per batch, asynchronous
 *                 aclhip_peer_close_buffer(ctx, peer)
 * The destination copies its own shard with the same call on its own pointer. The caller orders the destination's reads after the
 * pushes (a barrier between the processes, or events it shares). No reference counterpart (the reference is single threaded CPU code). */
#define ACLHIP_PEER_HANDLE_BYTES 72
aclhip_status aclhip_peer_export_buffer(aclhip_context* context, void* device_buffer, uint8_t* out_handle);
aclhip_status aclhip_peer_open_buffer(aclhip_context* context, const uint8_t* handle, void** out_device_buffer);
aclhip_status aclhip_peer_close_buffer(aclhip_context* context, void* device_buffer);
aclhip_status aclhip_push_poses_to_peer(aclhip_context* context, void* peer_buffer, uint64_t offset_bytes, const void* shard_poses, uint64_t shard_bytes, void* stream);

/* Number of instances the kernels refused since the context was created (unknown clip handle, track index out of range):
 * the reference silently returns in those cases (impl/decompression.transform.h:1532-1537,1766-1768). */
aclhip_status aclhip_get_rejected_instance_count(aclhip_context* context, uint64_t* out_count);

/* Number of transforms the pose consumers combined through rtm::qvv_mul's MATRIX route (local -> object space, the `relative`
 * additive format) because a NEGATIVE scale component was involved, since the context was created: mirrored rigs, for which RTM
 * composes 3x4 matrices instead of quaternions, and so do the kernels (qvv_mul_through_matrices, bit for bit the oracle's restatement;
 * pinned by an fp64 matrix chain in tests/test_pose_consumers_oracle.py). The route is compiled into a launch only while some
 * registered clip can decode a negative scale (found at registration from defaults, constants, clip ranges and raw segments) or the
 * base is a caller's pose buffer. 0 for every rig with non-negative scales. Waits for the device like
 * aclhip_get_rejected_instance_count. */
aclhip_status aclhip_get_negative_scale_count(aclhip_context* context, uint64_t* out_count);

/* ---- measurement helpers ---------------------------------------------------------------------- */

/* Runs `repeats` launches of aclhip_decompress_tracks_batch on `stream` bracketed by HIP events recorded on that same
 * stream and returns the average milliseconds per launch (device time of the decode kernel, no host overhead). */
aclhip_status aclhip_time_decompress_tracks_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, void* poses, uint64_t pose_stride_bytes, void* stream, uint32_t repeats, float* out_ms_per_launch);

/* Same for aclhip_decompress_poses_batch. */
aclhip_status aclhip_time_decompress_poses_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, void* poses, uint64_t pose_stride_bytes, void* stream, uint32_t repeats, float* out_ms_per_launch);

/* Name of the kernel aclhip_decompress_tracks_batch would launch for `params` with the clips registered so far, for pose rows as wide
 * as the largest registered clip (to match rocprofv3 kernel traces with bench results). */
aclhip_status aclhip_describe_tracks_kernel(aclhip_context* context, const aclhip_decompress_params* params, char* out_name, uint32_t capacity);

/* The same for the launch aclhip_decompress_tracks_batch_out makes with `output` (may be NULL) and rows of `pose_stride_bytes`: the kernel's
 * name and (optional) the wavefronts per instance -- answered by the functions the launch itself asks. */
aclhip_status aclhip_describe_tracks_launch(aclhip_context* context, const aclhip_decompress_params* params, const aclhip_output_desc* output, uint64_t pose_stride_bytes,
	char* out_name, uint32_t capacity, uint32_t* out_windows_per_instance);

/* Streams `size_bytes` of 16 byte per lane stores into `buffer` (DEVICE pointer, 16 byte aligned) `repeats` times and returns the
 * GB/s reached: the practical ceiling of a pose shaped write stream on this device, to read roofline fractions against. */
aclhip_status aclhip_measure_write_bandwidth(aclhip_context* context, void* buffer, uint64_t size_bytes, uint32_t repeats, void* stream, float* out_gb_per_second);

/* The write stream of a pose batch ALONE: one wave per pose window storing the window's rows with the pose kernels' own 1 KiB streaming
 * stores into `poses` (DEVICE pointer; num_instances rows of pose_stride_bytes, num_tracks 48 byte records each), nothing decoded,
 * at 32 / 16 / 12 / 8 resident waves per CU and with 0 / 3 / 6 dependent scalar loads pacing every wave, and the runtime's own fill of
 * the same bytes (hipMemsetAsync). Returns the best rate (and the occupancy that reached it; 0 = the runtime's fill): the BEST MEASURED
 * STORE-ONLY RATE over this buffer among those thirteen shapes -- a second denominator to read a decode's roofline fraction against
 * besides the 8 TB/s of the specification, not a bound: a decode whose stores are paced differently can come out above it.
 * OVERWRITES `poses`. Measurement aid (bench.py: roofline.best_store_only_gbps). */
aclhip_status aclhip_measure_pose_store_bandwidth(aclhip_context* context, void* poses, uint64_t pose_stride_bytes, uint32_t num_instances, uint32_t num_tracks,
	uint32_t repeats, void* stream, float* out_gb_per_second, uint32_t* out_waves_per_cu);

/* Algorithmic bytes of one batch under the compulsory-HBM model of DESIGN.md: poses written plus each distinct
 * clip's touched bytes once. `clips` is a HOST pointer here. */
aclhip_status aclhip_batch_algorithmic_bytes(const aclhip_context* context, const aclhip_clip* clips, uint32_t num_instances,
	uint64_t* out_bytes_written, uint64_t* out_distinct_clip_bytes);

#if defined(__cplusplus)
}
#endif

#endif
