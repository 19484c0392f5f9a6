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
	// the slot's track, or the fill -- a filled slot takes the same arithmetic as a decoded one. combine(slot, kind, value, what the image holds)
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
			image[slot_quad] = combine(slot, kind, value, image[slot_quad]);
		}
	}

	// strength: full_strength, or under aclhip_additive_layering an additive_strength
	template<class strength_type = full_strength>
	__device__ __forceinline__ void apply_additive_clip_onto_slot_image(const device_clip& clip, const device_track_map& map, const slot_fill& fill, float sample_time,
		uint32_t rounding_policy, const decode_params& params, uint32_t additive_format, uint32_t lane, f32x4* image, const strength_type& strength = {})
	{
		combine_constant_slots(clip, map, fill, lane, image, [&](uint32_t slot, uint32_t kind, float4 value, f32x4 base) { return apply_additive_sub_track(additive_format, kind, strength(slot, kind, value), base); });
		decode_animated_into_image(clip, sample_time, rounding_policy, params, lane, into_slots(map, additive_image_writer<false, strength_type>{ image, additive_format, strength }));
	}

	// weight: uniform_weight, or under blend masks a slot_weight
	template<class weight_type>
	__device__ __forceinline__ void blend_clip_onto_slot_image(const device_clip& clip, const device_track_map& map, const slot_fill& fill, float sample_time,
		uint32_t rounding_policy, const decode_params& params, const weight_type& weight, uint32_t lane, f32x4* image)
	{
		combine_constant_slots(clip, map, fill, lane, image, [&](uint32_t slot, uint32_t kind, float4 value, f32x4 accumulated) { return blend_accumulate(kind, accumulated, value, weight(slot)); });
		decode_animated_into_image(clip, sample_time, rounding_policy, params, lane, into_slots(map, blend_image_writer<weight_type>{ image, weight }));
	}

	// blend_partners_refused's track test in skeleton space: the partner's own map (skeleton_launch::blend_maps), known, made for this clip and
	// for a skeleton of this many bones
	__device__ __forceinline__ bool blend_map_fits(const skeleton_launch* mapping, size_t entry, const ACLHIP_CONSTANT device_clip* record, uint32_t num_bones)
	{
		const uint32_t blend_map_id = as_constant(mapping->blend_maps)[entry];
		const ACLHIP_CONSTANT device_track_map* map_record = as_constant(mapping->maps) + (blend_map_id < mapping->num_maps ? blend_map_id : 0);
		return blend_map_id < mapping->num_maps && map_record->image != nullptr && map_record->num_tracks == record->num_tracks && map_record->num_slots == num_bones;
	}

	// ---- blend masks (aclhip_register_blend_mask, aclhip_decompress_poses_batch_masked) ------------------------------------------------
	// A weight per (instance, clip, SLOT) in the place of the blend's weight per (instance, clip): include/aclhip.h states the definition.
	// A mask's record in the context's mask table (which never moves, like the map table) and its device image: num_slots floats in slot
	// order. A cleared record (image == null) is an unknown or retired mask; record 0 is never handed out (handle 0: no mask).
	struct device_blend_mask
	{
		const float* image;
		uint32_t num_slots;
		uint32_t reserved;
	};
	static_assert(sizeof(device_blend_mask) == 16, "one dwordx4 load");

	// the masked kernels' own trailing argument, behind skeleton_launch
	struct blend_mask_launch
	{
		const device_blend_mask* masks;			// the context's mask table
		uint32_t num_masks;						// its capacity
		uint32_t layered;						// ACLHIP_BLEND_LAYERED
		const uint32_t* instance_masks;			// [num_instances * K], laid out like consumer_params::blend_weights; 0: no mask
	};

	// The weight of ONE clip of a masked blend at a slot. The pointers and the clip weights are wave uniform (read on the scalar unit next
	// to the clip and map records); the mask values are read per lane through the vector cache, like track_to_slot: a mask is a few
	// hundred bytes that every wave of a crowd reads. above1 .. above3: the layers over this clip in layered mode, the TOP one first -- the
	// order the definition multiplies (1 - e_j) in. A layer that is not there (fewer than three above, or weighted mode) has no mask and
	// weight 0: r * (1 - 0) is r, so the product is the definition's bit for bit, and e * 1 is e. (Named fields, not arrays: an array of
	// pointers here went to scratch in the instantiations with a second wave.)
	// blend_poses_kernel (kernels_pose_buffers.inl) restates slot_weight's product as ONE running product over its K layers, top layer first,
	// so that every mask value is read once: a change to the arithmetic here has to be made there as well.
	struct layer_weight
	{
		const ACLHIP_CONSTANT float* mask;		// null: no mask, every slot 1
		float weight;
		__device__ __forceinline__ float operator()(uint32_t slot) const { return mask != nullptr ? weight * mask[slot] : weight; }
	};

	struct slot_weight
	{
		layer_weight own, above1, above2, above3;
		__device__ __forceinline__ float operator()(uint32_t slot) const
		{
			const float opacity = own(slot);
			float rest = 1.0f - above1(slot);
			rest = rest * (1.0f - above2(slot));
			rest = rest * (1.0f - above3(slot));
			return opacity * rest;
		}
	};
	static_assert(ACLHIP_MAX_BLEND_CLIPS == 4, "slot_weight: at most three layers above a clip");

	// (the mask behind a handle the kernel has checked: known, of the skeleton's slot count -- or the null handle)
	__device__ __forceinline__ layer_weight layer_weight_of(const device_blend_mask* masks, const ACLHIP_CONSTANT uint32_t* handles, const ACLHIP_CONSTANT float* weights, uint32_t k)
	{
		const uint32_t handle = handles[k];
		// (the pointer alone: two scalar registers per layer, not a record's four)
		return layer_weight{ handle != 0 ? as_constant(as_constant(masks)[handle].image) : nullptr, weights[k] };
	}

	// clip k's weight of an instance (`handles`, `weights`: the instance's K entries): its own mask and weight and, in layered mode, those
	// of the clips above it
	__device__ __forceinline__ slot_weight slot_weight_of(const device_blend_mask* masks, uint32_t layered, const ACLHIP_CONSTANT uint32_t* handles, const ACLHIP_CONSTANT float* weights,
		uint32_t num_blend_clips, uint32_t k)
	{
		slot_weight result;
		result.own = layer_weight_of(masks, handles, weights, k);
		const uint32_t num_above = layered != 0 ? num_blend_clips - 1u - k : 0u;
		result.above1 = result.above2 = result.above3 = layer_weight{ nullptr, 0.0f };
		if (num_above > 0)
			result.above1 = layer_weight_of(masks, handles, weights, num_blend_clips - 1u);
		if (num_above > 1)
			result.above2 = layer_weight_of(masks, handles, weights, num_blend_clips - 2u);
		if (num_above > 2)
			result.above3 = layer_weight_of(masks, handles, weights, num_blend_clips - 3u);
		return result;
	}

	// A map's and a skeleton's record with every field in scalar registers of its own, like load_clip_fields (kernels_pose.inl): load_entry
	// hands back two 4 register blocks, a block lives as long as ANY of its fields and is spilled whole -- in the masked kernels with a
	// second wave such a spill left a 16 byte stack slot behind that nothing read or wrote, and a kernel with a stack gets scratch memory
	__device__ __forceinline__ device_track_map load_map_fields(const device_track_map* table, uint32_t index)
	{
		device_track_map map = load_entry(table, index);
		asm volatile("" : "+s"(map.image), "+s"(map.num_tracks), "+s"(map.num_slots), "+s"(map.num_unmapped));
		return map;
	}

	__device__ __forceinline__ device_skeleton load_skeleton_fields(const device_skeleton* table, uint32_t index)
	{
		device_skeleton skeleton = load_entry(table, index);
		asm volatile("" : "+s"(skeleton.hierarchy), "+s"(skeleton.reference_pose), "+s"(skeleton.num_bones), "+s"(skeleton.flags));
		return skeleton;
	}

	// The masked kernels' arguments as they lie in the kernarg segment (in order, each at its natural alignment), like pose_kernel_args
	// (kernels_pose.inl): what the blend's passes and the tail of the kernel need -- the lists of the blend, the tables, where the pose
	// goes -- is read THERE, where it is used, instead of being held (spilled) in scalar registers across up to four decodes.
	struct masked_kernel_args
	{
		const device_clip* clips;
		uint32_t num_clips;
		const uint32_t* clip_ids;
		const float* sample_times;
		uint32_t num_instances;
		decode_params params;
		consumer_params consumers;
		uint8_t* poses;
		uint64_t pose_stride_bytes;
		uint32_t lds_quads_per_image;
		uint32_t lds_bytes_per_instance;
		uint32_t packed_block_shape;
		unsigned long long* rejected_count;
		skeleton_launch mapping;
		blend_mask_launch masking;
	};
	// (the offsets the compiler's kernel metadata lists for decompress_poses_masked_kernel: tools/kernel_resources.sh's assembly, `.offset`)
	static_assert(offsetof(masked_kernel_args, params) == 40 && offsetof(masked_kernel_args, consumers) == 160 && offsetof(masked_kernel_args, poses) == 232
		&& offsetof(masked_kernel_args, lds_quads_per_image) == 248 && offsetof(masked_kernel_args, rejected_count) == 264 && offsetof(masked_kernel_args, mapping) == 272
		&& offsetof(masked_kernel_args, masking) == 336 && sizeof(masked_kernel_args) == 360, "masked_kernel_args mirrors the kernel's argument list");
	// the bounds instantiations' trailing argument behind them (aclhip_decompress_poses_batch_bounds)
	struct masked_bounds_kernel_args
	{
		masked_kernel_args launch;
		consumer_bounds_launch bounds;
	};
	static_assert(offsetof(masked_bounds_kernel_args, bounds) == 360 && sizeof(masked_bounds_kernel_args) == 376, "masked_bounds_kernel_args mirrors the kernel's argument list");

	__device__ __forceinline__ decode_params load_decode_params(const ACLHIP_CONSTANT decode_params* source)
	{
		decode_params params;
		__builtin_memcpy(&params, (const ACLHIP_CONSTANT void*)source, sizeof(params));
		return params;
	}

	// (opaque per use: not hoisted to the kernel's start and kept across the decodes)
	__device__ __forceinline__ const ACLHIP_CONSTANT masked_kernel_args* late_masked_kernel_args()
	{
	#if defined(__HIP_DEVICE_COMPILE__)
		const ACLHIP_CONSTANT masked_kernel_args* args = (const ACLHIP_CONSTANT masked_kernel_args*)__builtin_amdgcn_kernarg_segment_ptr();
		asm volatile("" : "+s"(args));
		return args;
	#else
		return nullptr;		// (the host pass only has to compile)
	#endif
	}

	// ---- additive strength (aclhip_additive_layering, aclhip_decompress_poses_batch_additive_weighted) ---------------------------------
	// A strength per (instance, SLOT) on the additive pose in front of apply_additive_to_base: include/aclhip.h states the definition. The
	// masks are the blend masks (device_blend_mask, the context's table).
	// the additive kernels' own trailing argument, behind skeleton_launch
	struct additive_strength_launch
	{
		const device_blend_mask* masks;			// the context's mask table
		uint32_t num_masks;						// its capacity
		uint32_t reserved;
		const float* instance_weights;			// [num_instances] or null: every instance 1
		const uint32_t* instance_masks;			// [num_instances] or null; 0: no mask
	};

	// The strength of an instance's additive layer: layer_weight gives e = w, or w * mask[slot] through the vector cache (one load per quad);
	// the pointer, the weight and the two settings are wave uniform.
	struct additive_strength
	{
		layer_weight weight;
		uint32_t additive_format;
		uint32_t short_exact;		// the instance's walk_may_use_short_exact_math verdict, and w in [0, 1] (masks are: aclhip_register_blend_mask)
		__device__ __forceinline__ float4 operator()(uint32_t slot, uint32_t kind, float4 value) const
		{
			const float strength = weight(slot);
			return short_exact != 0 ? weigh_additive_sub_track<true>(additive_format, kind, value, strength) : weigh_additive_sub_track<false>(additive_format, kind, value, strength);
		}
	};

	// The additive kernels' arguments as they lie in the kernarg segment, like masked_kernel_args: the layering is read THERE, where the
	// strength is made -- behind the base clip's decode in the fused instantiations, behind every decode in the others.
	struct additive_kernel_args
	{
		const device_clip* clips;
		uint32_t num_clips;
		const uint32_t* clip_ids;
		const float* sample_times;
		uint32_t num_instances;
		decode_params params;
		consumer_params consumers;
		uint8_t* poses;
		uint64_t pose_stride_bytes;
		uint32_t lds_quads_per_image;
		uint32_t lds_bytes_per_instance;
		uint32_t packed_block_shape;
		unsigned long long* rejected_count;
		skeleton_launch mapping;
		additive_strength_launch layering;
	};
	static_assert(offsetof(additive_kernel_args, mapping) == offsetof(masked_kernel_args, mapping) && offsetof(additive_kernel_args, layering) == 336 && sizeof(additive_kernel_args) == 368,
		"additive_kernel_args mirrors the kernel's argument list");

	// (opaque per use, like late_masked_kernel_args)
	__device__ __forceinline__ const ACLHIP_CONSTANT additive_strength_launch* late_additive_layering()
	{
	#if defined(__HIP_DEVICE_COMPILE__)
		const ACLHIP_CONSTANT additive_kernel_args* args = (const ACLHIP_CONSTANT additive_kernel_args*)__builtin_amdgcn_kernarg_segment_ptr();
		asm volatile("" : "+s"(args));
		return &args->layering;
	#else
		return nullptr;		// (the host pass only has to compile)
	#endif
	}

	// (the mask behind a handle the kernel has checked: known, of the skeleton's slot count -- or the null handle)
	__device__ __forceinline__ additive_strength additive_strength_of(uint32_t instance, uint32_t additive_format, uint32_t short_exact)
	{
		const ACLHIP_CONSTANT additive_strength_launch* layering = late_additive_layering();
		const float weight = layering->instance_weights != nullptr ? as_constant(layering->instance_weights)[instance] : 1.0f;
		const uint32_t handle = layering->instance_masks != nullptr ? as_constant(layering->instance_masks)[instance] : 0u;
		const ACLHIP_CONSTANT float* mask = handle != 0 ? as_constant(as_constant(layering->masks)[handle].image) : nullptr;
		return additive_strength{ layer_weight{ mask, weight }, additive_format, (weight >= 0.0f && weight <= 1.0f) ? short_exact : 0u };
	}

	// ---- one body for the mapped and the additive entry points ---------------------------------------------------------------------------
	// decompress_poses_skeleton_kernel and decompress_poses_additive_kernel are decompress_poses_consumer_kernel (kernels_consumers.inl: the
	// workgroup's shape, the LDS layout, the walk and the store are described there) in skeleton space, with the mapping as a trailing
	// argument: decode_params, consumer_params and every kernarg offset are where that kernel has them. They run ONE text,
	// skeleton_space_poses -- the refusal test takes the skeleton and the maps in, the images are filled in slot order, and behind the decodes
	// it is that kernel's finish_consumer_poses, without rotation | translation images and without ACLHIP_CONSUMERS_FAST -- and hand it a
	// policy for the little that differs between them:
	//   refuses()      the entry point's own refusal next to the inherited ones: nothing, or the mask handle of an additive layering
	//   strength()     what an additive clip is weighed with: full_strength (nothing), or the instance's additive_strength -- and whether
	//                  an additive image that is not fused with its base is weighed behind the blend (k_weighs_additive_image)
	//   bounds         the bounds instantiations' trailing argument (the mapped kernel's policy only: the additive kernel has no bounds form)
	// decompress_poses_masked_kernel (below) calls consumer_wave_of, mapped_instance_of, mapped_instance_refused, resolve_base_clip and the
	// functions the body calls, not the body: on the body, or with the second wave's decode or the refuse / serve ladder inside shared
	// functions, instantiations of it lost a wave per SIMD or got scratch (profiles/skeleton_kernel_sharing.md has the figures).

	// An instance of a mapped launch: its clip (every field in registers of its own: load_clip_fields, kernels_pose.inl), its skeleton and its
	// clip's map, read on the scalar unit next to the clip record. A cleared record (an unknown or retired handle) holds no image; record 0
	// of both tables is never handed out.
	struct mapped_instance
	{
		uint32_t clip_id, skeleton_id, map_id;
		device_clip clip;
		device_skeleton skeleton;
		device_track_map clip_map;
	};
	__device__ __forceinline__ mapped_instance mapped_instance_of(const device_clip* clips, uint32_t num_clips, const uint32_t* clip_ids, const skeleton_launch* mapping, uint32_t instance)
	{
		mapped_instance the;
		the.clip_id = as_constant(clip_ids)[instance];
		the.clip = load_clip_fields(clips, the.clip_id < num_clips ? the.clip_id : 0);
		the.skeleton_id = mapping->instance_skeletons != nullptr ? as_constant(mapping->instance_skeletons)[instance] : mapping->skeleton;
		the.map_id = mapping->instance_maps != nullptr ? as_constant(mapping->instance_maps)[instance] : mapping->map;
		the.skeleton = load_skeleton_fields(mapping->skeletons, the.skeleton_id < mapping->num_skeletons ? the.skeleton_id : 0);
		the.clip_map = load_map_fields(mapping->maps, the.map_id < mapping->num_maps ? the.map_id : 0);
		return the;
	}

	// refused: unknown / scalar clips, unknown or retired skeletons and maps, a map made for another clip or another skeleton, object
	// space without a hierarchy, more bones than the row or the launch's LDS image holds, and what the entry point's policy refuses
	// (unknown or retired masks, masks of another slot count). Both waves of an instance come to the same verdict; the first one
	// reports it. A launch is shaped for its batch when it is enqueued (launch_consumers: LDS image sizes from the pose stride, kernel
	// instantiation from what the registry holds) and meets its clips and skeletons when it runs: a clip or a reference pose that may
	// hand a negative scale to a launch compiled without rtm::qvv_mul's matrix route -- registered behind a captured launch's back --
	// is refused here, not computed wrongly. Only launches that MULTIPLY transforms care: local space without a base, and additive0 /
	// additive1 onto a fused base clip, combine scale with scale and serve mirrored skeletons as they are.
	template<bool kObjectSpace, uint32_t kBase, bool kMirrored>
	__device__ __forceinline__ bool mapped_instance_refused(uint32_t clip_id, uint32_t num_clips, const device_clip& clip, uint32_t skeleton_id, const device_skeleton& skeleton, uint32_t map_id,
		const device_track_map& clip_map, const skeleton_launch* mapping, uint64_t pose_stride_bytes, uint32_t lds_quads_per_image, uint64_t base_pose_stride_bytes)
	{
		constexpr bool base_is_clip = kBase == k_consumer_base_second_wave || kBase == k_consumer_base_fused;
		constexpr bool multiplies_transforms = kObjectSpace || kBase == k_consumer_base_buffer || kBase == k_consumer_base_second_wave;
		const uint32_t pose_tracks = skeleton.num_bones;
		return clip_id >= num_clips || !is_transform_clip(clip.flags) || (kObjectSpace && skeleton.hierarchy == nullptr)
			|| skeleton_id >= mapping->num_skeletons || skeleton.reference_pose == nullptr || !map_fits(clip_map, map_id, mapping->num_maps, clip.num_tracks, skeleton.num_bones)
			|| uint64_t(pose_tracks) * 48u > pose_stride_bytes || pose_tracks * 3u > lds_quads_per_image
			|| (kBase == k_consumer_base_buffer && uint64_t(pose_tracks) * 48u > base_pose_stride_bytes)
			|| (!kMirrored && multiplies_transforms && (skeleton.flags & k_skeleton_negative_scale) != 0)
			|| (!kMirrored && multiplies_transforms && !base_is_clip && (clip.flags & k_clip_negative_scale) != 0);
	}

	// The base clip of an instance (consumer_params::base_clip_ids) and its own map (skeleton_launch::base_maps): each clip only has to match
	// its own map, each map the skeleton. (The second wave's decode of the base stays with the callers: inside this function it cost
	// instantiations a wave per SIMD or gave them scratch, profiles/skeleton_kernel_sharing.md.)
	struct base_records
	{
		device_clip clip;
		device_track_map map;
	};
	template<bool kObjectSpace, uint32_t kBase, bool kMirrored>
	__device__ __forceinline__ base_records resolve_base_clip(const device_clip* clips, uint32_t num_clips, const consumer_params& consumers, const skeleton_launch* mapping, uint32_t instance,
		const device_clip& clip, const device_skeleton& skeleton, const decode_params& params, bool& refused, uint32_t& short_exact)
	{
		constexpr bool multiplies_transforms = kObjectSpace || kBase == k_consumer_base_buffer || kBase == k_consumer_base_second_wave;
		const uint32_t base_clip_id = as_constant(consumers.base_clip_ids)[instance];
		const device_clip base_clip = load_clip_fields(clips, base_clip_id < num_clips ? base_clip_id : 0);
		const uint32_t base_map_id = as_constant(mapping->base_maps)[instance];
		const device_track_map base_map = load_map_fields(mapping->maps, base_map_id < mapping->num_maps ? base_map_id : 0);
		refused = refused || base_clip_id >= num_clips || !is_transform_clip(base_clip.flags) || !map_fits(base_map, base_map_id, mapping->num_maps, base_clip.num_tracks, skeleton.num_bones)
			|| (!kMirrored && multiplies_transforms && ((clip.flags | base_clip.flags) & k_clip_negative_scale) != 0);
		short_exact &= walk_may_use_short_exact_math(base_clip.flags, params.normalization);
		return base_records{ base_clip, base_map };
	}

	// the leading arguments the mapped kernels share and the mapping, as the kernel holds them
	struct mapped_kernel_launch
	{
		const device_clip* clips;
		uint32_t num_clips;
		const uint32_t* clip_ids;
		const float* sample_times;
		uint32_t num_instances;
		const decode_params& params;
		const consumer_params& consumers;
		uint8_t* poses;
		uint64_t pose_stride_bytes;
		uint32_t lds_quads_per_image, lds_bytes_per_instance, packed_block_shape;
		unsigned long long* rejected_count;
		const skeleton_launch& mapping;
	};

	// decompress_poses_skeleton_kernel's policy: nothing of its own. bounds: the bounds instantiations' trailing argument, or null
	struct mapped_poses_policy
	{
		static constexpr bool k_weighs_additive_image = false;
		const consumer_bounds_launch* bounds = nullptr;
		__device__ __forceinline__ bool refuses(uint32_t, uint32_t) const { return false; }
		__device__ __forceinline__ full_strength strength(uint32_t, uint32_t, uint32_t) const { return {}; }
	};

	// decompress_poses_additive_kernel's: the instance's mask record is checked next to its maps, and the strength goes in at one of two
	// places. Fused (additive0 / additive1 onto a base clip, one image): on every additive sub-track in front of apply_additive_sub_track --
	// one quad is still touched by one lane per pass. Otherwise (a second wave's image, a base pose buffer, a blend) the additive pose sits
	// complete in its own image: one pass over it, behind the blend's normalize and in front of finish_consumer_poses' barrier. The layering
	// is read from the kernarg segment (additive_kernel_args).
	struct additive_poses_policy
	{
		static constexpr bool k_weighs_additive_image = true;
		__device__ __forceinline__ bool refuses(uint32_t instance, uint32_t num_bones) const
		{
			const ACLHIP_CONSTANT additive_strength_launch* layering = late_additive_layering();
			const uint32_t mask_id = layering->instance_masks != nullptr ? as_constant(layering->instance_masks)[instance] : 0u;
			const ACLHIP_CONSTANT device_blend_mask* mask_record = as_constant(layering->masks) + (mask_id < layering->num_masks ? mask_id : 0);
			return mask_id != 0 && (mask_id >= layering->num_masks || mask_record->image == nullptr || mask_record->num_slots != num_bones);
		}
		__device__ __forceinline__ additive_strength strength(uint32_t instance, uint32_t additive_format, uint32_t short_exact) const
		{
			return additive_strength_of(instance, additive_format, short_exact);
		}
	};

	template<bool kObjectSpace, uint32_t kBase, bool kMirrored, bool kBlend, bool kBounds, class policy_type>
	__device__ __forceinline__ void skeleton_space_poses(const mapped_kernel_launch& launch, const policy_type& policy, consumer_walk_slots& walk)
	{
		static_assert(!kBlend || kBase != k_consumer_base_fused, "a blend accumulates whole qvv images; a base clip is decoded by a second wave");
		constexpr bool base_is_clip = kBase == k_consumer_base_second_wave || kBase == k_consumer_base_fused;
		// a base clip under additive0 / additive1: ONE wave decodes the base into the instance's image and the additive clip onto it
		// (half the LDS per instance, half the waves: twice the poses a CU holds); otherwise a second wave decodes the base into its own image
		constexpr bool fused_base = kBase == k_consumer_base_fused;
		constexpr bool two_waves = kBase == k_consumer_base_second_wave;
		constexpr bool object_space = kObjectSpace;
		const skeleton_launch* const mapping = &launch.mapping;
		const consumer_params& consumers = launch.consumers;
		const device_clip* const clips = launch.clips;
		const uint32_t num_clips = launch.num_clips;
		const uint64_t pose_stride_bytes = launch.pose_stride_bytes;
		const uint32_t lds_quads_per_image = launch.lds_quads_per_image;
		// packed_block_shape: log2 of the instances per workgroup (bits 0..7) | words of LDS reserved for the shared walk schedule (bits 8..31)
		const uint32_t log2_instances_per_block = launch.packed_block_shape & 0xFFu;
		ACLHIP_PHASE_STAMP(0);

		consumer_wave wave = consumer_wave_of(log2_instances_per_block, launch.lds_bytes_per_instance, lds_quads_per_image);
		const uint32_t lane = wave.lane, role = wave.role, instance = wave.instance;
		f32x4* const image = wave.image;

		// (wave.num_tracks stays 0 for a wave without work: past the batch, refused instance, empty track list)
		// the walk's normalize may take the short exact forms when every rotation it meets comes out of clips that are proven safe for
		// them (norms near 1; a caller's base pose buffer holds anything)
		uint32_t short_exact = kBase == k_consumer_base_buffer ? 0u : 1u;
		if (instance < launch.num_instances)
		{
			const mapped_instance the = mapped_instance_of(clips, num_clips, launch.clip_ids, mapping, instance);
			const uint32_t clip_id = the.clip_id, skeleton_id = the.skeleton_id, map_id = the.map_id;
			const device_clip& clip = the.clip;
			const device_skeleton& skeleton = the.skeleton;
			const device_track_map& clip_map = the.clip_map;
			// the transforms of the instance's pose and the hierarchy they are walked with are the skeleton's (clip.hierarchy is not read)
			const uint32_t pose_tracks = skeleton.num_bones;
			const uint32_t* const hierarchy = skeleton.hierarchy;

			constexpr bool multiplies_transforms = object_space || kBase == k_consumer_base_buffer || kBase == k_consumer_base_second_wave;
			bool refused = mapped_instance_refused<kObjectSpace, kBase, kMirrored>(clip_id, num_clips, clip, skeleton_id, skeleton, map_id, clip_map, mapping, pose_stride_bytes, lds_quads_per_image,
				consumers.base_pose_stride_bytes);

			const uint32_t rounding_policy = __builtin_amdgcn_readfirstlane(instance_rounding_policy_of(launch.params, instance));
			// the instance's own looping policy (decompress.h:149) goes for every clip decoded on its behalf -- its base, its blend partners
			decode_params params = launch.params;
			params.looping_policy = uint8_t(__builtin_amdgcn_readfirstlane(instance_looping_policy_of(launch.params, instance)));

			short_exact &= walk_may_use_short_exact_math(clip.flags, params.normalization);
			short_exact &= (skeleton.flags & k_skeleton_short_exact_math) != 0 ? 1u : 0u;		// (the reference pose fills slots: its rotations are walked too)
			// what a slot no track maps to holds: the reference pose -- or, for an additive clip and its blend partners, the additive identity
			const slot_fill clip_fill = slot_fill_of(skeleton, consumers.additive_format);
			device_clip base_clip = clip;
			device_track_map base_map = {};
			if constexpr (base_is_clip)
			{
				const base_records base = resolve_base_clip<kObjectSpace, kBase, kMirrored>(clips, num_clips, consumers, mapping, instance, clip, skeleton, params, refused, short_exact);
				base_clip = base.clip;
				base_map = base.map;
				if (!refused && two_waves && role == 1 && pose_tracks != 0)
					decode_pose_into_slot_image(base_clip, base_map, slot_fill{ skeleton.reference_pose, 0 }, as_constant(consumers.base_sample_times)[instance], rounding_policy, params, lane, wave.base_image);
			}

			// every clip of the blend: known, a transform clip, with a known map of its own into this skeleton
			if (!refused)
			{
				if constexpr (kBlend)
					refused = blend_partners_refused<!kMirrored && multiplies_transforms>(clips, num_clips, consumers, instance, params.normalization, short_exact,
						[&](size_t entry, const ACLHIP_CONSTANT device_clip* record) { return blend_map_fits(mapping, entry, record, skeleton.num_bones); });
				refused = refused || policy.refuses(instance, skeleton.num_bones);
			}

			if (refused)
			{
				if (lane == 0 && role == 0)
					atomicAdd(launch.rejected_count, 1ull);
			}
			else if (pose_tracks != 0)
			{
				wave.num_tracks = pose_tracks;
				if (role == 0)
				{
					if (object_space)
						request_walk_schedule(hierarchy, log2_instances_per_block, launch.packed_block_shape >> 8, wave.shared_schedule, wave.slot, lane, walk);
					if constexpr (fused_base)
					{
						decode_pose_into_slot_image(base_clip, base_map, slot_fill{ skeleton.reference_pose, 0 }, as_constant(consumers.base_sample_times)[instance], rounding_policy, params, lane, image);
						wave_lds_barrier();		// the base pose is complete (its DMA has landed)
						apply_additive_clip_onto_slot_image(clip, clip_map, clip_fill, as_constant(launch.sample_times)[instance], rounding_policy, params, consumers.additive_format, lane, image,
							policy.strength(instance, consumers.additive_format, short_exact));
					}
					else
					{
						decode_pose_into_slot_image(clip, clip_map, clip_fill, as_constant(launch.sample_times)[instance], rounding_policy, params, lane, image);
						if constexpr (kBlend)
						{
							const uint32_t num_blend_clips = consumers.num_blend_clips;
							const ACLHIP_CONSTANT float* weights = as_constant(consumers.blend_weights) + size_t(instance) * num_blend_clips;
							wave_lds_barrier();		// the first pose is complete (its DMA has landed)
							blend_scale_image(image, pose_tracks * 3u, uniform_weight{ weights[0] }, lane);
							for (uint32_t k = 1; k < num_blend_clips; ++k)
							{
								const size_t entry = size_t(instance) * (num_blend_clips - 1u) + (k - 1u);
								const device_clip blend_clip = load_clip_fields(clips, as_constant(consumers.blend_clip_ids)[entry]);
								wave_lds_barrier();		// every quad has its sum so far
								const device_track_map blend_map = load_map_fields(mapping->maps, as_constant(mapping->blend_maps)[entry]);
								blend_clip_onto_slot_image(blend_clip, blend_map, clip_fill, as_constant(consumers.blend_sample_times)[entry], rounding_policy, params, uniform_weight{ weights[k] }, lane, image);
							}
							wave_lds_barrier();
							blend_normalize_rotations(image, pose_tracks, lane);
						}
						if constexpr (policy_type::k_weighs_additive_image)
						{
							wave_lds_barrier();		// the additive pose is complete (its DMA has landed; a blend's rotations are normalized)
							weigh_additive_image(image, pose_tracks * 3u, policy.strength(instance, consumers.additive_format, short_exact), lane);
						}
					}
				}
			}
			else if constexpr (kBounds)
				wave.empty_pose = true;		// (a served instance whose pose has no transform)
		}

		// both images of every instance are complete
		wave.short_exact = short_exact;
		consumer_bounds_launch bounds = bounds_launch_of();
		if constexpr (kBounds)
			bounds = bounds_launch_of(*policy.bounds);
		finish_consumer_poses<kObjectSpace, kBase, false, kMirrored, false, kBounds>(
			consumer_tail_args{ launch.poses, launch.pose_stride_bytes, launch.lds_bytes_per_instance, log2_instances_per_block, launch.rejected_count, consumers.base_poses, consumers.base_pose_stride_bytes,
				consumers.additive_format, bounds.bounds, bounds.bone_flags },
			wave, walk);
	}

	// (the bounds instantiations' trailing argument: nothing, or consumer_bounds_launch -- aclhip_decompress_poses_batch_bounds, kernels_consumers.inl)
	__device__ __forceinline__ const consumer_bounds_launch* bounds_argument_of() { return nullptr; }
	__device__ __forceinline__ const consumer_bounds_launch* bounds_argument_of(const consumer_bounds_launch& launch) { return &launch; }

	// aclhip_decompress_poses_batch_mapped
	template<bool kObjectSpace, uint32_t kBase, bool kMirrored, bool kBlend, class... bounds_types>
	__global__ __launch_bounds__(k_consumer_max_waves * k_wave_size) void decompress_poses_skeleton_kernel(const device_clip* __restrict__ clips, uint32_t num_clips,
		const uint32_t* __restrict__ clip_ids, const float* __restrict__ sample_times, uint32_t num_instances, decode_params launch_params, consumer_params consumers,
		uint8_t* __restrict__ poses, uint64_t pose_stride_bytes, uint32_t lds_quads_per_image, uint32_t lds_bytes_per_instance, uint32_t packed_block_shape,
		unsigned long long* __restrict__ rejected_count, skeleton_launch skeleton_mapping, bounds_types... bounds_launch)
	{
		__shared__ consumer_walk_slots walk;		// (what the host subtracts from the LDS it may ask for: host_consumers.inl)
		skeleton_space_poses<kObjectSpace, kBase, kMirrored, kBlend, sizeof...(bounds_types) != 0>(
			mapped_kernel_launch{ clips, num_clips, clip_ids, sample_times, num_instances, launch_params, consumers, poses, pose_stride_bytes, lds_quads_per_image, lds_bytes_per_instance, packed_block_shape, rejected_count, skeleton_mapping },
			mapped_poses_policy{ bounds_argument_of(bounds_launch...) }, walk);
	}

	// skeleton_space_poses' blend instantiations with a weight per slot (aclhip_decompress_poses_batch_masked), the masking as their own
	// trailing argument, in a text of their own (see above). What differs from that body: the K mask records are checked next to the K maps; the three places
	// that take a weight -- the first clip's scale, the constant / fill pass, the animated writer -- are handed a slot_weight; and what the
	// blend's passes and finish_consumer_poses need of the launch is read late, from the kernarg segment (masked_kernel_args). One quad
	// is still touched by one lane per pass: the LDS hazards and the barriers are that body's.
	template<bool kObjectSpace, uint32_t kBase, bool kMirrored, class... bounds_types>
	__global__ __launch_bounds__(k_consumer_max_waves * k_wave_size) void decompress_poses_masked_kernel(const device_clip* __restrict__ clips, uint32_t num_clips,
		const uint32_t* __restrict__ clip_ids, const float* __restrict__ sample_times, uint32_t num_instances, decode_params launch_params, consumer_params consumers,
		uint8_t* __restrict__ poses, uint64_t pose_stride_bytes, uint32_t lds_quads_per_image, uint32_t lds_bytes_per_instance, uint32_t packed_block_shape,
		unsigned long long* __restrict__ rejected_count, skeleton_launch skeleton_mapping, blend_mask_launch blend_masking, bounds_types...)
	{
		// (bounds_types: nothing, or consumer_bounds_launch, read where the box is stored: masked_bounds_kernel_args)
		constexpr bool with_bounds = sizeof...(bounds_types) != 0;
		const skeleton_launch* const mapping = &skeleton_mapping;
		const blend_mask_launch* const masking = &blend_masking;
		(void)poses;		// (read where the pose is stored: masked_kernel_args)
		// (registers of their own, like load_map_fields: the three arrive in one dwordx4 load of the kernarg segment, and in the instantiations
		// with a second wave the block's spill slot stayed behind as 16 bytes of stack that nothing read or wrote)
		asm volatile("" : "+s"(lds_quads_per_image), "+s"(lds_bytes_per_instance), "+s"(packed_block_shape));
		// packed_block_shape: log2 of the instances per workgroup (bits 0..7) | words of LDS reserved for the shared walk schedule (bits 8..31)
		const uint32_t log2_instances_per_block = packed_block_shape & 0xFFu;
		__shared__ consumer_walk_slots walk;		// (what the host subtracts from the LDS it may ask for: host_consumers.inl)

		static_assert(kBase != k_consumer_base_fused, "a blend accumulates whole qvv images; a base clip is decoded by a second wave");
		// (a blend's base clip is never fused: a second wave decodes it into its own image)
		constexpr bool base_is_clip = kBase == k_consumer_base_second_wave;
		constexpr bool two_waves = base_is_clip;
		constexpr bool object_space = kObjectSpace;
		ACLHIP_PHASE_STAMP(0);

		const consumer_wave layout = consumer_wave_of(log2_instances_per_block, lds_bytes_per_instance, lds_quads_per_image);
		const uint32_t lane = layout.lane, wave_in_block = layout.wave_in_block, slot = layout.slot, role = layout.role, instance = layout.instance;
		f32x4* const image = layout.image;
		f32x4* const base_image = layout.base_image;
		uint32_t* const shared_schedule = layout.shared_schedule;

		uint32_t num_tracks = 0;		// stays 0 for a wave without work: past the batch, refused instance, empty track list
		// the walk's normalize may take the short exact forms when every rotation it meets comes out of clips that are proven safe for
		// them (norms near 1; a caller's base pose buffer holds anything)
		uint32_t short_exact = kBase == k_consumer_base_buffer ? 0u : 1u;
		[[maybe_unused]] bool empty_pose = false;		// (bounds: a served instance whose pose has no transform)
		if (instance < num_instances)
		{
			const mapped_instance the = mapped_instance_of(clips, num_clips, clip_ids, mapping, instance);
			const uint32_t clip_id = the.clip_id, skeleton_id = the.skeleton_id, map_id = the.map_id;
			const device_clip& clip = the.clip;
			const device_skeleton& skeleton = the.skeleton;
			const device_track_map& clip_map = the.clip_map;
			// the transforms of the instance's pose and the hierarchy they are walked with are the skeleton's (clip.hierarchy is not read)
			const uint32_t pose_tracks = skeleton.num_bones;
			const uint32_t* const hierarchy = skeleton.hierarchy;

			// refused: unknown or retired masks and masks of another slot count (below, next to the blend's maps), and everything
			// mapped_instance_refused refuses
			constexpr bool multiplies_transforms = object_space || kBase == k_consumer_base_buffer || kBase == k_consumer_base_second_wave;
			bool refused = mapped_instance_refused<kObjectSpace, kBase, kMirrored>(clip_id, num_clips, clip, skeleton_id, skeleton, map_id, clip_map, mapping, pose_stride_bytes, lds_quads_per_image,
				consumers.base_pose_stride_bytes);

			const uint32_t rounding_policy = __builtin_amdgcn_readfirstlane(instance_rounding_policy_of(launch_params, instance));
			// the instance's own looping policy (decompress.h:149) goes for every clip decoded on its behalf -- its base, its blend partners
			decode_params params = launch_params;
			const uint8_t looping_policy = uint8_t(__builtin_amdgcn_readfirstlane(instance_looping_policy_of(launch_params, instance)));
			params.looping_policy = looping_policy;

			short_exact &= walk_may_use_short_exact_math(clip.flags, params.normalization);
			short_exact &= (skeleton.flags & k_skeleton_short_exact_math) != 0 ? 1u : 0u;		// (the reference pose fills slots: its rotations are walked too)
			// what a slot no track maps to holds: the reference pose -- or, for an additive clip and its blend partners, the additive identity
			const slot_fill clip_fill = slot_fill_of(skeleton, consumers.additive_format);
			if constexpr (base_is_clip)
			{
				const base_records base = resolve_base_clip<kObjectSpace, kBase, kMirrored>(clips, num_clips, consumers, mapping, instance, clip, skeleton, params, refused, short_exact);
				if (!refused && two_waves && role == 1 && pose_tracks != 0)
					decode_pose_into_slot_image(base.clip, base.map, slot_fill{ skeleton.reference_pose, 0 }, as_constant(consumers.base_sample_times)[instance], rounding_policy, params, lane, base_image);
			}

			if (!refused)
			{
				// every clip of the blend: known, a transform clip, with a known map of its own into this skeleton
				refused = blend_partners_refused<!kMirrored && multiplies_transforms>(clips, num_clips, consumers, instance, params.normalization, short_exact,
					[&](size_t entry, const ACLHIP_CONSTANT device_clip* record) { return blend_map_fits(mapping, entry, record, skeleton.num_bones); });
				// every mask the instance names: the null handle, or a known mask of this skeleton's slot count
				for (uint32_t k = 0; k < consumers.num_blend_clips; ++k)
				{
					const uint32_t mask_id = as_constant(masking->instance_masks)[size_t(instance) * consumers.num_blend_clips + k];
					const ACLHIP_CONSTANT device_blend_mask* mask_record = as_constant(masking->masks) + (mask_id < masking->num_masks ? mask_id : 0);
					refused = refused || (mask_id != 0 && (mask_id >= masking->num_masks || mask_record->image == nullptr || mask_record->num_slots != skeleton.num_bones));
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
						request_walk_schedule(hierarchy, log2_instances_per_block, packed_block_shape >> 8, shared_schedule, slot, lane, walk);
					decode_pose_into_slot_image(clip, clip_map, clip_fill, as_constant(sample_times)[instance], rounding_policy, params, lane, image);
					{
						// (every pass reads its lists and tables from the kernarg segment: masked_kernel_args)
						const uint32_t num_blend_clips = consumers.num_blend_clips;
						wave_lds_barrier();		// the first pose is complete (its DMA has landed)
						{
							const ACLHIP_CONSTANT masked_kernel_args* args = late_masked_kernel_args();
							blend_scale_image(image, pose_tracks * 3u, slot_weight_of(args->masking.masks, args->masking.layered, as_constant(args->masking.instance_masks) + size_t(instance) * num_blend_clips,
								as_constant(args->consumers.blend_weights) + size_t(instance) * num_blend_clips, num_blend_clips, 0), lane);
						}
						for (uint32_t k = 1; k < num_blend_clips; ++k)
						{
							const ACLHIP_CONSTANT masked_kernel_args* args = late_masked_kernel_args();
							const size_t entry = size_t(instance) * (num_blend_clips - 1u) + (k - 1u);
							const device_clip blend_clip = load_clip_fields(args->clips, as_constant(args->consumers.blend_clip_ids)[entry]);
							wave_lds_barrier();		// every quad has its sum so far
							const device_track_map blend_map = load_map_fields(args->mapping.maps, as_constant(args->mapping.blend_maps)[entry]);
							const slot_weight weight = slot_weight_of(args->masking.masks, args->masking.layered, as_constant(args->masking.instance_masks) + size_t(instance) * num_blend_clips,
								as_constant(args->consumers.blend_weights) + size_t(instance) * num_blend_clips, num_blend_clips, k);
							// (the launch's decode settings too, with the instance's looping policy as above)
							decode_params pass_params = load_decode_params(&args->params);
							pass_params.looping_policy = looping_policy;
							blend_clip_onto_slot_image(blend_clip, blend_map, clip_fill, as_constant(args->consumers.blend_sample_times)[entry], rounding_policy, pass_params, weight, lane, image);
						}
						wave_lds_barrier();
						blend_normalize_rotations(image, pose_tracks, lane);
					}
				}
			}
			else if constexpr (with_bounds)
				empty_pose = true;
		}

		// both images of every instance are complete
		// (what the tail needs of the launch is read from the kernarg segment here, behind the decodes: masked_kernel_args)
		const ACLHIP_CONSTANT masked_kernel_args* const tail_args = late_masked_kernel_args();
		consumer_bounds_launch bounds = bounds_launch_of();
		if constexpr (with_bounds)
		{
			const ACLHIP_CONSTANT consumer_bounds_launch* late_bounds = &reinterpret_cast<const ACLHIP_CONSTANT masked_bounds_kernel_args*>(tail_args)->bounds;
			bounds = bounds_launch_of(consumer_bounds_launch{ late_bounds->bounds, late_bounds->bone_flags });
		}
		finish_consumer_poses<kObjectSpace, kBase, false, kMirrored, false, with_bounds>(
			consumer_tail_args{ tail_args->poses, tail_args->pose_stride_bytes, tail_args->lds_bytes_per_instance, log2_instances_per_block, tail_args->rejected_count,
				tail_args->consumers.base_poses, tail_args->consumers.base_pose_stride_bytes, tail_args->consumers.additive_format, bounds.bounds, bounds.bone_flags },
			consumer_wave{ image, base_image, shared_schedule, slot, role, lane, wave_in_block, instance, num_tracks, short_exact, empty_pose }, walk);
	}

	// aclhip_decompress_poses_batch_additive_weighted: the additive instantiations with a strength per (instance, slot) on the additive pose,
	// the layering as their own trailing argument (read from the kernarg segment: additive_kernel_args)
	template<bool kObjectSpace, uint32_t kBase, bool kMirrored, bool kBlend>
	__global__ __launch_bounds__(k_consumer_max_waves * k_wave_size) void decompress_poses_additive_kernel(const device_clip* __restrict__ clips, uint32_t num_clips,
		const uint32_t* __restrict__ clip_ids, const float* __restrict__ sample_times, uint32_t num_instances, decode_params launch_params, consumer_params consumers,
		uint8_t* __restrict__ poses, uint64_t pose_stride_bytes, uint32_t lds_quads_per_image, uint32_t lds_bytes_per_instance, uint32_t packed_block_shape,
		unsigned long long* __restrict__ rejected_count, skeleton_launch skeleton_mapping, additive_strength_launch)
	{
		static_assert(kBase != k_consumer_base_none, "an additive layer goes onto a base");
		__shared__ consumer_walk_slots walk;
		skeleton_space_poses<kObjectSpace, kBase, kMirrored, kBlend, false>(
			mapped_kernel_launch{ clips, num_clips, clip_ids, sample_times, num_instances, launch_params, consumers, poses, pose_stride_bytes, lds_quads_per_image, lds_bytes_per_instance, packed_block_shape, rejected_count, skeleton_mapping },
			additive_poses_policy{}, walk);
	}
