// kernels_skeleton.inl -- part of aclhip.hip (one translation unit; included there behind kernels_consumers.inl, not compiled on its own).
// Skeleton space for the pose consumers (aclhip_decompress_poses_batch_mapped): decompress_poses_skeleton_kernel builds its LDS image in
// SLOT order from the start -- every clip of an instance lands in it through its own track map, slots no track maps to are filled --
// and everything behind the decode is decompress_poses_consumer_kernel's with the skeleton's bone count and walk schedule.

	// ---- skeletons (aclhip_register_skeleton) ---------------------------------------------------------------------------------------------
	// A skeleton's record in the context's skeleton table (which never moves, like the clip table and the map table). A cleared record
	// (reference_pose == null) is an unknown or retired skeleton.
	struct device_skeleton
	{
		const uint32_t* hierarchy;			// the walk schedule image aclhip_set_clip_hierarchy builds, in slot order; null: local space only
		const f32x4* reference_pose;		// [3 * num_bones] rotation | translation | scale per bone (the W of translations and scales is 0)
		uint32_t num_bones;
		uint32_t flags;						// k_skeleton_*
		uint32_t reserved[2];
	};
	static_assert(sizeof(device_skeleton) == 32, "load_entry: two dwordx4 loads");
	constexpr uint32_t k_skeleton_negative_scale = 1u << 0;		// the reference pose holds a scale below zero: rtm::qvv_mul's matrix route may be taken
	constexpr uint32_t k_skeleton_short_exact_math = 1u << 1;	// every rotation of the reference pose has a squared length in [1/4, 4]: the walk's short exact normalize applies

	// the mapped consumer kernels' own trailing argument
	struct skeleton_launch
	{
		const device_skeleton* skeletons;		// the context's skeleton table
		const device_track_map* maps;			// the context's map table
		uint32_t num_skeletons;					// their capacities
		uint32_t num_maps;
		uint32_t skeleton;						// the launch's skeleton, when instance_skeletons is null
		uint32_t map;							// the launch's map (of clips[i]), when instance_maps is null
		const uint32_t* instance_skeletons;		// [num_instances] or null
		const uint32_t* instance_maps;			// [num_instances] or null
		const uint32_t* blend_maps;				// [num_instances * (K - 1)], laid out like consumer_params::blend_clip_ids
		const uint32_t* base_maps;				// [num_instances]
	};

	// The additive identity per sub-track kind (compression/impl/compress.transform.impl.h:422: what the reference's compressor
	// takes for the default sub-tracks of an additive clip): scale 1 for relative and additive0, scale 0 for additive1
	__device__ const f32x4 k_additive_identity_quads[6] =
	{
		{ 0.0f, 0.0f, 0.0f, 1.0f }, { 0.0f, 0.0f, 0.0f, 0.0f }, { 1.0f, 1.0f, 1.0f, 0.0f },
		{ 0.0f, 0.0f, 0.0f, 1.0f }, { 0.0f, 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f, 0.0f },
	};

	// What a slot no track maps to holds, as a table of quads: indexed by the quad of the pose (the reference pose) or by its kind alone
	struct slot_fill
	{
		const f32x4* table;
		uint32_t per_kind;
		__device__ __forceinline__ const f32x4* quad(uint32_t slot_quad, uint32_t kind) const { return table + (per_kind != 0 ? kind : slot_quad); }
	};

	// the fill of the instance's own clip and of its blend partners (a base clip always fills with the reference pose)
	__device__ __forceinline__ slot_fill slot_fill_of(const device_skeleton& skeleton, uint32_t additive_format)
	{
		if (additive_format == ACLHIP_ADDITIVE_NONE)
			return slot_fill{ skeleton.reference_pose, 0 };
		return slot_fill{ k_additive_identity_quads + (additive_format == ACLHIP_ADDITIVE_ADDITIVE1 ? 3 : 0), 1 };
	}

	// a known map of this clip into this skeleton?
	__device__ __forceinline__ bool map_fits(const device_track_map& map, uint32_t map_id, uint32_t num_maps, uint32_t clip_tracks, uint32_t num_bones)
	{
		return map_id < num_maps && map.image != nullptr && map.num_tracks == clip_tracks && map.num_slots == num_bones;
	}

	__device__ __forceinline__ const ACLHIP_CONSTANT uint32_t* slot_to_track_of(const device_track_map& map)
	{
		return as_constant(map.image) + map.num_tracks + map.num_unmapped;
	}

	// A decoded sub-track of track t goes where the unmapped writer would put it for track map[t]; dropped tracks go nowhere.
	// track_to_slot is read per lane through the vector cache: a map is a few hundred bytes that every wave of the launch reads, so it
	// stays in the L1 / L2, while a copy staged in LDS would take a barrier per clip (a blend decodes up to four) and LDS that decides
	// how many poses a CU holds.
	template<class image_writer_type>
	struct slot_image_writer
	{
		image_writer_type write_to_image;
		const ACLHIP_CONSTANT uint32_t* track_to_slot;
		__device__ __forceinline__ void operator()(const clip_range_entry& entry, float4 value) const
		{
			const uint32_t slot = track_to_slot[entry.track_index];
			if (slot == ACLHIP_TRACK_DROPPED)
				return;
			clip_range_entry moved = entry;
			moved.track_index = slot;
			moved.quad_index = slot * 3u + (entry.quad_index - entry.track_index * 3u);
			write_to_image(moved, value);
		}
	};

	template<class image_writer_type>
	__device__ __forceinline__ slot_image_writer<image_writer_type> into_slots(const device_track_map& map, image_writer_type write_to_image)
	{
		return slot_image_writer<image_writer_type>{ write_to_image, as_constant(map.image) };
	}

	// decode_pose_into_image in slot order: ONE gathered DMA, lanes <-> quads of the num_slots x 3 image, the source of a mapped slot its
	// track's quad of the clip's resolved pose, of any other slot the fill; then the animated sub-tracks through the map.
	__device__ __forceinline__ void decode_pose_into_slot_image(const device_clip& clip, const device_track_map& map, const slot_fill& fill, float sample_time,
		uint32_t rounding_policy, const decode_params& params, uint32_t lane, f32x4* image)
	{
		const uint32_t num_quads = map.num_slots * 3u;
		const ACLHIP_CONSTANT uint32_t* slot_to_track = slot_to_track_of(map);
		const f32x4* resolved = reinterpret_cast<const f32x4*>(clip.resolved_pose);
		for (uint32_t base = 0; base < num_quads; base += k_wave_size)
		{
			const uint32_t slot_quad = base + lane;
			if (slot_quad < num_quads)
			{
				const uint32_t slot = slot_quad / 3u;
				const uint32_t kind = slot_quad - slot * 3u;
				const uint32_t track = slot_to_track[slot];
				const f32x4* source = track != ACLHIP_TRACK_DROPPED ? resolved + (track * 3u + kind) : fill.quad(slot_quad, kind);
				__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)source,
					(__attribute__((address_space(3))) void*)(image + base), 16, 0, 0);
			}
		}
		decode_animated_into_image(clip, sample_time, rounding_policy, params, lane, into_slots(map, qvv48_image_writer{ image, 0, 0xFFFFFFFFu }));
	}

	// The constant / default pass of blend_clip_onto_image and apply_additive_clip_onto_image over SLOTS: the base pose table entry of
	// the slot's track, or the fill -- a filled slot takes the same arithmetic as a decoded one
	template<class combine_type>
	__device__ __forceinline__ void combine_constant_slots(const device_clip& clip, const device_track_map& map, const slot_fill& fill, uint32_t lane, f32x4* image, combine_type combine)
	{
		const uint32_t num_quads = map.num_slots * 3u;
		const ACLHIP_CONSTANT uint32_t* slot_to_track = slot_to_track_of(map);
		for (uint32_t slot_quad = lane; slot_quad < num_quads; slot_quad += k_wave_size)
		{
			const uint32_t slot = slot_quad / 3u;
			const uint32_t kind = slot_quad - slot * 3u;
			const uint32_t track = slot_to_track[slot];
			float4 value;
			if (track != ACLHIP_TRACK_DROPPED)
			{
				value = load_quad(clip.base_pose, track * 3u + kind);
				const uint32_t marker = __float_as_uint(value.w);
				if (is_special_quad(marker))
				{
					if ((marker & k_quad_animated) != 0)
						continue;
					value.w = (marker & k_quad_default_w_one) != 0 ? 1.0f : 0.0f;
				}
			}
			else
			{
				const f32x4 filled = *fill.quad(slot_quad, kind);
				value = make_float4(filled.x, filled.y, filled.z, filled.w);
			}
			image[slot_quad] = combine(kind, value, image[slot_quad]);
		}
	}

	__device__ __forceinline__ void apply_additive_clip_onto_slot_image(const device_clip& clip, const device_track_map& map, const slot_fill& fill, float sample_time,
		uint32_t rounding_policy, const decode_params& params, uint32_t additive_format, uint32_t lane, f32x4* image)
	{
		combine_constant_slots(clip, map, fill, lane, image, [&](uint32_t kind, float4 value, f32x4 base) { return apply_additive_sub_track(additive_format, kind, value, base); });
		decode_animated_into_image(clip, sample_time, rounding_policy, params, lane, into_slots(map, additive_image_writer<>{ image, additive_format }));
	}

	__device__ __forceinline__ void blend_clip_onto_slot_image(const device_clip& clip, const device_track_map& map, const slot_fill& fill, float sample_time,
		uint32_t rounding_policy, const decode_params& params, float weight, uint32_t lane, f32x4* image)
	{
		combine_constant_slots(clip, map, fill, lane, image, [&](uint32_t kind, float4 value, f32x4 accumulated) { return blend_accumulate(kind, accumulated, value, weight); });
		decode_animated_into_image(clip, sample_time, rounding_policy, params, lane, into_slots(map, blend_image_writer{ image, weight }));
	}

	// decompress_poses_consumer_kernel (kernels_consumers.inl: the workgroup's shape, the LDS layout, the walk and the store are described
	// there) in skeleton space, with the mapping as its own trailing argument: decode_params, consumer_params and every kernarg offset
	// are where that kernel has them. A kernel of its own rather than a flag of that one: every way of sharing the text that was tried
	// (a common device function, one body under two entry points) moved registers in 29 of the 32 existing instantiations, and those
	// are held to identical disassembly (profiles/skeleton_poses.md). No rotation | translation images, no ACLHIP_CONSUMERS_FAST.
	// What that kernel keeps for them is not repeated here.
	template<bool kObjectSpace, uint32_t kBase, bool kMirrored, bool kBlend>
	__global__ __launch_bounds__(k_consumer_max_waves * k_wave_size) void decompress_poses_skeleton_kernel(const device_clip* __restrict__ clips, uint32_t num_clips,
		const uint32_t* __restrict__ clip_ids, const float* __restrict__ sample_times, uint32_t num_instances, decode_params launch_params, consumer_params consumers,
		uint8_t* __restrict__ poses, uint64_t pose_stride_bytes, uint32_t lds_quads_per_image, uint32_t lds_bytes_per_instance, uint32_t packed_block_shape,
		unsigned long long* __restrict__ rejected_count, skeleton_launch skeleton_mapping)
	{
		const skeleton_launch* const mapping = &skeleton_mapping;
		// packed_block_shape: log2 of the instances per workgroup (bits 0..7) | words of LDS reserved for the shared walk schedule (bits 8..31)
		const uint32_t log2_instances_per_block = packed_block_shape & 0xFFu;
		extern __shared__ __attribute__((aligned(16))) uint8_t dynamic_lds[];
		__shared__ consumer_walk_slots walk;		// (what the host subtracts from the LDS it may ask for: host_consumers.inl)
		uint32_t (&walk_levels)[k_consumer_max_instances] = walk.levels;
		const uint32_t* (&walk_schedules)[k_consumer_max_instances] = walk.schedules;
		uint32_t (&walk_tracks)[k_consumer_max_instances] = walk.tracks;
		uint32_t (&walk_short_exact)[k_consumer_max_instances] = walk.short_exact;

		static_assert(!kBlend || kBase != k_consumer_base_fused, "a blend accumulates whole qvv images; a base clip is decoded by a second wave");
		constexpr bool has_base = kBase != k_consumer_base_none;
		constexpr bool base_is_clip = kBase == k_consumer_base_second_wave || kBase == k_consumer_base_fused;
		// a base clip under additive0 / additive1: ONE wave decodes the base into the instance's image and the additive clip onto it
		// (half the LDS per instance, half the waves: twice the poses a CU holds); otherwise a second wave decodes the base into its own image
		constexpr bool fused_base = kBase == k_consumer_base_fused;
		constexpr bool two_waves = kBase == k_consumer_base_second_wave;
		constexpr bool object_space = kObjectSpace;
		ACLHIP_PHASE_STAMP(0);

		// wave -> (instance slot of the workgroup, role): role 1 waves (base clips only) decode the slot's base
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		const uint32_t slot = wave_in_block & ((1u << log2_instances_per_block) - 1u);
		const uint32_t role = wave_in_block >> log2_instances_per_block;
		const uint32_t waves_per_instance = two_waves ? 2u : 1u;
		const uint32_t instance = (blockIdx.x << log2_instances_per_block) + slot;

		uint8_t* instance_lds = dynamic_lds + size_t(slot) * lds_bytes_per_instance;
		f32x4* image = reinterpret_cast<f32x4*>(instance_lds);
		f32x4* base_image = image + lds_quads_per_image;
		// one LDS copy of the walk schedule per workgroup, behind the instances' images: the instances of a workgroup usually share
		// a skeleton (identical hierarchies are one image, see aclhip_set_clip_hierarchy), and every word kept per instance costs residency
		uint32_t* shared_schedule = reinterpret_cast<uint32_t*>(dynamic_lds + (size_t(lds_bytes_per_instance) << log2_instances_per_block));
		const uint32_t* schedule = nullptr;

		uint32_t num_tracks = 0;		// stays 0 for a wave without work: past the batch, refused instance, empty track list
		uint32_t num_levels = 0;
		// the walk's normalize may take the short exact forms when every rotation it meets comes out of clips that are proven safe for
		// them (norms near 1; a caller's base pose buffer holds anything)
		uint32_t short_exact = kBase == k_consumer_base_buffer ? 0u : 1u;
		if (instance < num_instances)
		{
			const uint32_t clip_id = as_constant(clip_ids)[instance];
			// (every field in registers of its own: load_clip_fields, kernels_pose.inl)
			const device_clip clip = load_clip_fields(clips, clip_id < num_clips ? clip_id : 0);

			// skeleton space: the instance's skeleton and its clip's map, read on the scalar unit next to the clip record. A cleared record
			// (an unknown or retired handle) holds no image; record 0 of both tables is never handed out.
			const uint32_t skeleton_id = mapping->instance_skeletons != nullptr ? as_constant(mapping->instance_skeletons)[instance] : mapping->skeleton;
			const uint32_t map_id = mapping->instance_maps != nullptr ? as_constant(mapping->instance_maps)[instance] : mapping->map;
			const device_skeleton skeleton = load_entry(mapping->skeletons, skeleton_id < mapping->num_skeletons ? skeleton_id : 0);
			const device_track_map clip_map = load_entry(mapping->maps, map_id < mapping->num_maps ? map_id : 0);
			// the transforms of the instance's pose and the hierarchy they are walked with are the skeleton's (clip.hierarchy is not read)
			const uint32_t pose_tracks = skeleton.num_bones;
			const uint32_t* const hierarchy = skeleton.hierarchy;

			// refused: unknown / scalar clips, unknown or retired skeletons and maps, a map made for another clip or another skeleton, object
			// space without a hierarchy, more bones than the row or the launch's LDS image holds. Both waves of an instance come to the same
			// verdict; the first one reports it. A launch is shaped for its batch when it is enqueued (launch_consumers: LDS image sizes from
			// the pose stride, kernel instantiation from what the registry holds) and meets its clips and skeletons when it runs: a clip or a
			// reference pose that may hand a negative scale to a launch compiled without rtm::qvv_mul's matrix route -- registered behind a
			// captured launch's back -- is refused here, not computed wrongly. Only launches that MULTIPLY transforms care: local space
			// without a base, and additive0 / additive1 onto a fused base clip, combine scale with scale and serve mirrored skeletons as they are.
			constexpr bool multiplies_transforms = object_space || kBase == k_consumer_base_buffer || kBase == k_consumer_base_second_wave;
			bool refused = clip_id >= num_clips || !is_transform_clip(clip.flags) || (object_space && hierarchy == nullptr)
				|| skeleton_id >= mapping->num_skeletons || skeleton.reference_pose == nullptr || !map_fits(clip_map, map_id, mapping->num_maps, clip.num_tracks, skeleton.num_bones)
				|| uint64_t(pose_tracks) * 48u > pose_stride_bytes || pose_tracks * 3u > lds_quads_per_image
				|| (kBase == k_consumer_base_buffer && uint64_t(pose_tracks) * 48u > consumers.base_pose_stride_bytes)
				|| (!kMirrored && multiplies_transforms && (skeleton.flags & k_skeleton_negative_scale) != 0)
				|| (!kMirrored && multiplies_transforms && !base_is_clip && (clip.flags & k_clip_negative_scale) != 0);

			const uint32_t rounding_policy = __builtin_amdgcn_readfirstlane(instance_rounding_policy_of(launch_params, instance));
			// the instance's own looping policy (decompress.h:149) goes for every clip decoded on its behalf -- its base, its blend partners
			decode_params params = launch_params;
			params.looping_policy = uint8_t(__builtin_amdgcn_readfirstlane(instance_looping_policy_of(launch_params, instance)));

			short_exact &= walk_may_use_short_exact_math(clip.flags, params.normalization);
			short_exact &= (skeleton.flags & k_skeleton_short_exact_math) != 0 ? 1u : 0u;		// (the reference pose fills slots: its rotations are walked too)
			// what a slot no track maps to holds: the reference pose -- or, for an additive clip and its blend partners, the additive identity
			const slot_fill clip_fill = slot_fill_of(skeleton, consumers.additive_format);
			device_clip base_clip = clip;
			device_track_map base_map = {};
			if (base_is_clip)
			{
				const uint32_t base_clip_id = as_constant(consumers.base_clip_ids)[instance];
				base_clip = load_clip_fields(clips, base_clip_id < num_clips ? base_clip_id : 0);
				// (each clip only has to match its own map, each map the skeleton)
				const uint32_t base_map_id = as_constant(mapping->base_maps)[instance];
				base_map = load_entry(mapping->maps, base_map_id < mapping->num_maps ? base_map_id : 0);
				refused = refused || base_clip_id >= num_clips || !is_transform_clip(base_clip.flags) || !map_fits(base_map, base_map_id, mapping->num_maps, base_clip.num_tracks, skeleton.num_bones)
					|| (!kMirrored && multiplies_transforms && ((clip.flags | base_clip.flags) & k_clip_negative_scale) != 0);
				short_exact &= walk_may_use_short_exact_math(base_clip.flags, params.normalization);
				if (!refused && two_waves && role == 1 && pose_tracks != 0)
					decode_pose_into_slot_image(base_clip, base_map, slot_fill{ skeleton.reference_pose, 0 }, as_constant(consumers.base_sample_times)[instance], rounding_policy, params, lane, base_image);
			}

			if (kBlend && !refused)
			{
				// every clip of the blend: known, a transform clip, with a known map of its own into this skeleton
				for (uint32_t k = 1; k < consumers.num_blend_clips; ++k)
				{
					const uint32_t blend_clip_id = as_constant(consumers.blend_clip_ids)[size_t(instance) * (consumers.num_blend_clips - 1u) + (k - 1u)];
					const ACLHIP_CONSTANT device_clip* record = as_constant(clips) + (blend_clip_id < num_clips ? blend_clip_id : 0);
					const uint32_t blend_map_id = as_constant(mapping->blend_maps)[size_t(instance) * (consumers.num_blend_clips - 1u) + (k - 1u)];
					const ACLHIP_CONSTANT device_track_map* map_record = as_constant(mapping->maps) + (blend_map_id < mapping->num_maps ? blend_map_id : 0);
					refused = refused || blend_clip_id >= num_clips || !is_transform_clip(record->flags)
						|| blend_map_id >= mapping->num_maps || map_record->image == nullptr || map_record->num_tracks != record->num_tracks || map_record->num_slots != skeleton.num_bones
						|| (!kMirrored && multiplies_transforms && (record->flags & k_clip_negative_scale) != 0);
					short_exact &= walk_may_use_short_exact_math(record->flags, params.normalization);
				}
			}

			if (refused)
			{
				if (lane == 0 && role == 0)
					atomicAdd(rejected_count, 1ull);
			}
			else if (pose_tracks != 0)
			{
				num_tracks = pose_tracks;
				if (role == 0)
				{
					if (object_space)
					{
						// The walk schedule for this many instances per workgroup, requested BEFORE the decode (until round 4 behind it: three
						// more dependent round trips -- offset, header, words -- at the end of every wave's chain, 1.7 of a decode's 6.3 us).
						// One scalar load for the schedule's header (aclhip_set_clip_hierarchy: {offset, steps, words, 0} per workgroup size,
						// in flight next to the seek's sample records), then the words travel global -> LDS by DMA while the pose is decoded:
						//     num_steps | words | step_end[num_steps] | transform | parent << 16 in step order, padded to whole 16 byte pieces
						// Every wave leaves its schedule in the shared copy: the same words when they share it (the copy is only used then).
						// A schedule longer than the launch reserved LDS for (a hierarchy set behind a captured launch's back) stays in
						// global memory and the walk reads it there.
						const u32x4 header = ((const ACLHIP_CONSTANT u32x4*)hierarchy)[log2_instances_per_block];
						schedule = hierarchy + header.x;
						num_levels = header.y;
						const uint32_t num_words = header.z;
						if (num_words <= (packed_block_shape >> 8))
						{
							for (uint32_t base = 0; base < num_words; base += k_wave_size * 4u)
								if (base + lane * 4u < num_words)
									__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(schedule + base + lane * 4u),
										(__attribute__((address_space(3))) void*)(shared_schedule + base), 16, 0, 0);
						}
						else
							num_levels |= 0x80000000u;
					}
					if (fused_base)
					{
						decode_pose_into_slot_image(base_clip, base_map, slot_fill{ skeleton.reference_pose, 0 }, as_constant(consumers.base_sample_times)[instance], rounding_policy, params, lane, image);
						wave_lds_barrier();		// the base pose is complete (its DMA has landed)
						apply_additive_clip_onto_slot_image(clip, clip_map, clip_fill, as_constant(sample_times)[instance], rounding_policy, params, consumers.additive_format, lane, image);
					}
					else
						decode_pose_into_slot_image(clip, clip_map, clip_fill, as_constant(sample_times)[instance], rounding_policy, params, lane, image);
					if constexpr (kBlend)
					{
						const uint32_t num_blend_clips = consumers.num_blend_clips;
						const ACLHIP_CONSTANT float* weights = as_constant(consumers.blend_weights) + size_t(instance) * num_blend_clips;
						wave_lds_barrier();		// the first pose is complete (its DMA has landed)
						blend_scale_image(image, pose_tracks * 3u, weights[0], lane);
						for (uint32_t k = 1; k < num_blend_clips; ++k)
						{
							const size_t entry = size_t(instance) * (num_blend_clips - 1u) + (k - 1u);
							const device_clip blend_clip = load_clip_fields(clips, as_constant(consumers.blend_clip_ids)[entry]);
							wave_lds_barrier();		// every quad has its sum so far
							const device_track_map blend_map = load_entry(mapping->maps, as_constant(mapping->blend_maps)[entry]);
							blend_clip_onto_slot_image(blend_clip, blend_map, clip_fill, as_constant(consumers.blend_sample_times)[entry], rounding_policy, params, weights[k], lane, image);
						}
						wave_lds_barrier();
						blend_normalize_rotations(image, pose_tracks, lane);
					}
				}
			}
		}

		// both images of every instance are complete
		if (two_waves)
			__syncthreads();
		else
			wave_lds_barrier();

		if (has_base && !fused_base)
		{
			const f32x4* base_source = base_is_clip ? base_image : reinterpret_cast<const f32x4*>(consumers.base_poses + uint64_t(instance) * consumers.base_pose_stride_bytes);
			for (uint32_t transform_index = role * k_wave_size + lane; transform_index < num_tracks; transform_index += waves_per_instance * k_wave_size)
			{
				const qvv additive = load_qvv(image, transform_index);
				const qvv base = load_qvv(base_source, transform_index);
				store_qvv(image, transform_index, apply_additive_to_base<kMirrored>(consumers.additive_format, base, additive));
				// additive_clip_format8::relative is a qvv_mul (core/additive_utils.h:128-160)
				if constexpr (kMirrored)
				{
					const uint64_t mirrored = __ballot(consumers.additive_format == 1 && qvv_mul_takes_matrix_path(additive, base));
					if (mirrored != 0 && lane == uint32_t(__builtin_ctzll(mirrored)))
						atomicAdd(rejected_count + 1, (unsigned long long)__builtin_popcountll(mirrored));
				}
			}
		}

		if (object_space)
		{
			if (lane == 0 && role == 0)
			{
				walk_levels[slot] = num_levels;
				walk_schedules[slot] = schedule;
				walk_tracks[slot] = num_tracks;
				walk_short_exact[slot] = num_tracks != 0 ? short_exact : 1u;
			}
			__syncthreads();
			ACLHIP_PHASE_STAMP(1);

			// ONE wave walks and then stores the workgroup's poses; the others are done and give their wave slots and registers back (a
			// pose waits in LDS for the walk about as long as its decode took: with every wave parked at a barrier the wave slots, not the
			// LDS, decided how many poses a CU holds). The walking wave rotates with the workgroup index: waves land on SIMDs by their
			// index inside the workgroup, and walks that all ran on a CU's first SIMD would queue there.
			if (wave_in_block != (blockIdx.x & ((blockDim.x / k_wave_size) - 1u)))
				return;
			{
				// lanes <-> (instance slot, transform of the current step): slot = lane % instances, lane / instances picks the slot's
				// transform inside the step. A transform's parent was scheduled in an earlier step: final by the time it is read.
				const uint32_t walk_slot = lane & ((1u << log2_instances_per_block) - 1u);
				const uint32_t first = lane >> log2_instances_per_block;
				f32x4* slot_image = reinterpret_cast<f32x4*>(dynamic_lds + size_t(walk_slot) * lds_bytes_per_instance);
				const uint32_t slot_steps = walk_levels[walk_slot] & 0x7FFFFFFFu;
				const bool slot_schedule_is_shared = (walk_levels[walk_slot] & 0x80000000u) == 0;
				const uint32_t* slot_schedule = walk_schedules[walk_slot];

				const auto walk = [&](const auto* schedule_words, auto short_exact_tag)
				{
					constexpr bool k_short_exact = decltype(short_exact_tag)::value;		// sqrt_rn_short / rcp_rn_short in the normalize (aclhip_device.h)
					const auto* pairs = schedule_words + 2u + slot_steps;
					uint32_t step_start = 0;
					for (uint32_t step = 0; __any(int(step < slot_steps)) != 0; ++step)
					{
						if (step < slot_steps)
						{
							const uint32_t step_end = schedule_words[2 + step];
							const uint32_t pair_index = step_start + first;
							if (pair_index < step_end)
							{
								const uint32_t pair = pairs[pair_index];		// transform | parent << 16
								const qvv child = load_qvv(slot_image, pair & 0xFFFFu), parent = load_qvv(slot_image, pair >> 16);
								qvv object;
								if constexpr (kMirrored)
								{
									const uint64_t mirrored = __ballot(qvv_mul_takes_matrix_path(child, parent));
									if (mirrored != 0 && lane == uint32_t(__builtin_ctzll(mirrored)))
										atomicAdd(rejected_count + 1, (unsigned long long)__builtin_popcountll(mirrored));
									object = qvv_mul(child, parent);
									if (mirrored != 0 && qvv_mul_takes_matrix_path(child, parent))
										object = qvv_mul_through_matrices(child, parent);
								}
								else
								{
									// neither a registered clip nor a reference pose can hand over a negative scale and the base is a clip:
									// products and sums of non negative scales -- nothing to count, nothing to route
									object = qvv_mul(child, parent);
								}
								object.rotation = quat_normalize<k_short_exact>(object.rotation);
								store_qvv(slot_image, pair & 0xFFFFu, object);
							}
							step_start = step_end;
						}
						wave_lds_barrier();
					}
				};

				// all instances that walk follow the same schedule? then the shared LDS copy is theirs; otherwise each reads its own
				// from global memory (rare: mixed skeletons inside one workgroup)
				// the rest of the workgroup waits for this wave: it goes first on its SIMD
				__builtin_amdgcn_s_setprio(3);
				const uint64_t walkers = __ballot(slot_steps != 0);
				if (walkers != 0)
				{
					const uint32_t leader = uint32_t(__builtin_ctzll(walkers));
					const uint64_t mine = reinterpret_cast<uint64_t>(slot_schedule);
					const uint64_t first_schedule = (uint64_t(__shfl(uint32_t(mine >> 32), int(leader))) << 32) | __shfl(uint32_t(mine), int(leader));
					const bool shared_copy = __all(int(slot_steps == 0 || (mine == first_schedule && slot_schedule_is_shared))) != 0;
					const bool short_exact_walk = __all(int(walk_short_exact[walk_slot] != 0)) != 0;
					const auto walk_with = [&](auto short_exact_tag)
					{
						if (shared_copy)
							walk(static_cast<const uint32_t*>(shared_schedule), short_exact_tag);
						else
							walk(as_constant(slot_schedule), short_exact_tag);
					};
					if (short_exact_walk)
						walk_with(std::true_type());
					else
						walk_with(std::false_type());
				}
				__builtin_amdgcn_s_setprio(0);
			}
			wave_lds_barrier();
			ACLHIP_PHASE_STAMP(2);

			const uint32_t instances_per_block = 1u << log2_instances_per_block;
			for (uint32_t store_slot = 0; store_slot < instances_per_block; ++store_slot)
			{
				const uint32_t slot_quads = walk_tracks[store_slot] * 3u;
				const f32x4* slot_image = reinterpret_cast<const f32x4*>(dynamic_lds + size_t(store_slot) * lds_bytes_per_instance);
				f32x4* slot_pose = reinterpret_cast<f32x4*>(poses + uint64_t((blockIdx.x << log2_instances_per_block) + store_slot) * pose_stride_bytes);
				for (uint32_t quad = lane; quad < slot_quads; quad += k_wave_size)
					store_streaming(&slot_pose[quad], slot_image[quad]);
			}
			ACLHIP_PHASE_STAMP(3);
			return;
		}
		else if (two_waves)
			__syncthreads();
		else
			wave_lds_barrier();

		const uint32_t num_quads = num_tracks * 3u;
		f32x4* pose = reinterpret_cast<f32x4*>(poses + uint64_t(instance) * pose_stride_bytes);
		for (uint32_t quad = role * k_wave_size + lane; quad < num_quads; quad += waves_per_instance * k_wave_size)
			store_streaming(&pose[quad], image[quad]);
		ACLHIP_PHASE_STAMP(3);
	}
