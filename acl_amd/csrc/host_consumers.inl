// host_consumers.inl -- part of aclhip.hip (one translation unit; included there, in this order, not compiled on its own).
// Host side: hierarchies and their walk schedules, pose consumer launches, host pointer convenience entry points.

// ---- pose consumers ------------------------------------------------------------------------------------------------

namespace
{
	// local_to_object_space (compression/transform_pose_utils.h:35-50) walks transforms in index order and needs parents first: any
	// order that keeps a parent ahead of its children gives the same bits. The consumer kernel takes up to P transforms per step,
	// P = 64 lanes / instances per workgroup, so the walk is scheduled on the host, once per hierarchy: at every step the P ready
	// transforms with the longest chain of descendants below them (Hu's algorithm: optimal for unit-time tasks on a forest). A
	// 100 bone character of 13 depths, 4-18 wide, takes 14 steps of 8 instead of 19 (12, its depth, at 16 per step).
	struct hierarchy_tree
	{
		std::vector<uint32_t> height;			// transforms on the longest chain from this one down to a leaf
		std::vector<uint32_t> first_child;		// [num_tracks + 1] into children
		std::vector<uint32_t> children;
		std::vector<uint8_t> is_root;
	};

	// false: transform out_misplaced does not follow its parent
	bool build_hierarchy_tree(const uint32_t* parent_indices, uint32_t num_tracks, hierarchy_tree& out, uint32_t& out_misplaced)
	{
		out.height.assign(num_tracks, 1);
		out.first_child.assign(size_t(num_tracks) + 1, 0);
		out.children.assign(num_tracks, 0);
		out.is_root.assign(num_tracks, 0);
		for (uint32_t i = 0; i < num_tracks; ++i)
		{
			// transform 0 is a root whatever its parent index says: the reference never reads it
			out.is_root[i] = (i == 0 || parent_indices[i] == ACLHIP_NO_PARENT) ? 1 : 0;
			if (out.is_root[i])
				continue;
			if (parent_indices[i] >= i)
			{
				out_misplaced = i;
				return false;
			}
			out.first_child[parent_indices[i] + 1]++;
		}
		for (uint32_t i = num_tracks; i-- > 1;)
			if (!out.is_root[i])
				out.height[parent_indices[i]] = std::max(out.height[parent_indices[i]], out.height[i] + 1);
		for (uint32_t i = 0; i < num_tracks; ++i)
			out.first_child[i + 1] += out.first_child[i];
		std::vector<uint32_t> cursor(out.first_child.begin(), out.first_child.end() - 1);
		for (uint32_t i = 1; i < num_tracks; ++i)
			if (!out.is_root[i])
				out.children[cursor[parent_indices[i]]++] = i;
		return true;
	}

	// out_transforms: every transform that has a parent, in the order it is computed; step s covers [out_step_end[s - 1], out_step_end[s])
	void schedule_hierarchy_walk(const hierarchy_tree& tree, uint32_t num_tracks, uint32_t transforms_per_step, std::vector<uint32_t>& out_step_end, std::vector<uint32_t>& out_transforms)
	{
		out_step_end.clear();
		out_transforms.clear();
		// ready transforms, the one with the longest chain below it (then the lowest index) on top
		const auto less_urgent = [&](uint32_t a, uint32_t b) { return tree.height[a] != tree.height[b] ? tree.height[a] < tree.height[b] : a > b; };
		std::vector<uint32_t> ready;
		for (uint32_t i = 0; i < num_tracks; ++i)
			if (tree.is_root[i])
				for (uint32_t c = tree.first_child[i]; c < tree.first_child[i + 1]; ++c)
					ready.push_back(tree.children[c]);
		std::make_heap(ready.begin(), ready.end(), less_urgent);
		std::vector<uint32_t> taken;
		while (!ready.empty())
		{
			taken.clear();
			while (!ready.empty() && taken.size() < transforms_per_step)
			{
				std::pop_heap(ready.begin(), ready.end(), less_urgent);
				taken.push_back(ready.back());
				ready.pop_back();
			}
			// their children become ready for the NEXT step
			for (uint32_t transform : taken)
			{
				out_transforms.push_back(transform);
				for (uint32_t c = tree.first_child[transform]; c < tree.first_child[transform + 1]; ++c)
				{
					ready.push_back(tree.children[c]);
					std::push_heap(ready.begin(), ready.end(), less_urgent);
				}
			}
			out_step_end.push_back(uint32_t(out_transforms.size()));
		}
	}

	// The device image of a hierarchy's walk schedules (clips: aclhip_set_clip_hierarchy; skeletons: aclhip_register_skeleton):
	// [{offset of the schedule, its steps, its words, 0 (first header: offset of the parent table)} for 1, 2, 4, 8 instances per workgroup: one 16 byte scalar load tells a wave
	// all it needs to request the copy] then per schedule, 16 byte aligned and padded to whole 16 byte pieces (it travels to LDS by DMA):
	// num_steps | words of this schedule | step_end[num_steps] | transform | parent << 16, in step order (16 bits each: the
	// consumers' LDS images end at about 3400 transforms; every word of the copy a wave keeps in LDS costs residency)
	// Behind the four schedules, where no schedule's word count reaches: the hierarchy's PARENT TABLE, one word per transform, parent
	// (0xFFFF: a root) | number of ancestors << 16 -- what the single bone requests in object space climb (kernels_bone_object.inl: the
	// schedules are in step order and cannot be indexed by bone). Its offset is the fourth word of the first header.
	// Returns the words of the longest of the four schedules.
	uint32_t build_walk_schedule_image(const hierarchy_tree& tree, const uint32_t* parent_indices, uint32_t num_tracks, std::vector<uint32_t>& image)
	{
		image.assign(16, 0);
		uint32_t max_schedule_words = 0;
		for (uint32_t log2_instances = 0; log2_instances < 4; ++log2_instances)
		{
			std::vector<uint32_t> step_end, pairs;
			schedule_hierarchy_walk(tree, num_tracks, 64u >> log2_instances, step_end, pairs);
			for (uint32_t& pair : pairs)
				pair |= parent_indices[pair] << 16;

			const uint32_t num_steps = uint32_t(step_end.size());
			const uint32_t header_words = 2 + num_steps;
			const uint32_t schedule_words = align_to_u32(header_words + uint32_t(pairs.size()), 4);
			const uint32_t offset = uint32_t(image.size());
			image[log2_instances * 4 + 0] = offset;
			image[log2_instances * 4 + 1] = num_steps;
			image[log2_instances * 4 + 2] = schedule_words;
			image.resize(size_t(offset) + schedule_words, 0);
			image[offset + 0] = num_steps;
			image[offset + 1] = schedule_words;
			std::copy(step_end.begin(), step_end.end(), image.begin() + offset + 2);
			std::copy(pairs.begin(), pairs.end(), image.begin() + offset + header_words);
			max_schedule_words = std::max(max_schedule_words, schedule_words);
		}
		const uint32_t parents_offset = uint32_t(image.size());
		image[3] = parents_offset;
		image.resize(size_t(parents_offset) + align_to_u32(num_tracks, 4), 0);
		for (uint32_t i = 0; i < num_tracks; ++i)
		{
			// (parents first: the parent's word is complete)
			const uint32_t ancestors = tree.is_root[i] ? 0u : (image[parents_offset + parent_indices[i]] >> 16) + 1u;
			image[parents_offset + i] = (tree.is_root[i] ? 0xFFFFu : parent_indices[i]) | (ancestors << 16);
		}
		return max_schedule_words;
	}

	// One device image per distinct hierarchy (context->hierarchies): a clip or a skeleton whose hierarchy is already on the device shares
	// that image. stage_hierarchy finds it or allocates and stages the upload of a new one (the caller finishes its uploads), then
	// keep_hierarchy counts the new user -- or drop_hierarchy gives a new image back when the uploads failed. The registry lock is held.
	struct staged_hierarchy
	{
		std::vector<uint32_t> canonical;		// the parent indices with every root spelled ACLHIP_NO_PARENT
		uint32_t* d_image = nullptr;
		bool is_shared = false;
	};

	// false: out of memory (d_image == nullptr) or the upload could not be staged
	bool stage_hierarchy(aclhip_context* context, const uint32_t* parent_indices, uint32_t num_tracks, const std::vector<uint32_t>& image, size_t& staging_used, staged_hierarchy& out)
	{
		out.canonical.assign(parent_indices, parent_indices + num_tracks);
		for (uint32_t i = 0; i < num_tracks; ++i)
			if (i == 0 || parent_indices[i] == ACLHIP_NO_PARENT)
				out.canonical[i] = ACLHIP_NO_PARENT;
		// (first: what this recycles may be the very image looked for below -- its last user retired it a moment ago -- and recycling
		// erases entries of the list the search walks. Round 3 searched first and could pick up a dangling entry: found by
		// tests/test_gpu_lifetime.py once the timing of its launches changed)
		collect_retired(context, false);

		for (aclhip_context::hierarchy_image& candidate : context->hierarchies)
			if (candidate.parents == out.canonical)
			{
				out.d_image = candidate.d_image;
				out.is_shared = true;
				return true;
			}
		// (a piece of a clip slab, uploaded on the context's copy stream: no allocation call and no copy that would stall the device)
		out.d_image = reinterpret_cast<uint32_t*>(allocate_clip_memory(context, image.size() * sizeof(uint32_t)));
		out.is_shared = false;
		if (out.d_image == nullptr)
			return false;
		return stage_upload(context, out.d_image, image.data(), image.size() * sizeof(uint32_t), staging_used);
	}

	void keep_hierarchy(aclhip_context* context, staged_hierarchy& staged)
	{
		for (aclhip_context::hierarchy_image& candidate : context->hierarchies)
			if (candidate.d_image == staged.d_image)
			{
				candidate.num_users++;
				return;
			}
		aclhip_context::hierarchy_image created;
		created.parents = std::move(staged.canonical);
		created.d_image = staged.d_image;
		created.num_users = 1;
		context->hierarchies.push_back(std::move(created));
	}

	void drop_hierarchy(aclhip_context* context, const staged_hierarchy& staged)
	{
		if (!staged.is_shared && staged.d_image != nullptr)
			free_clip_memory(context, staged.d_image);
	}
}

extern "C" aclhip_status aclhip_plan_hierarchy_walk(const uint32_t* parent_indices, uint32_t num_tracks, uint32_t transforms_per_step, uint32_t* out_steps, uint32_t* out_num_steps)
{
	if ((parent_indices == nullptr && num_tracks != 0) || out_num_steps == nullptr || transforms_per_step == 0)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return guarded(nullptr, [&]() -> aclhip_status
	{
		hierarchy_tree tree;
		uint32_t misplaced = 0;
		if (!build_hierarchy_tree(parent_indices, num_tracks, tree, misplaced))
			return ACLHIP_ERROR_INVALID_ARGUMENT;
		std::vector<uint32_t> step_end, transforms;
		schedule_hierarchy_walk(tree, num_tracks, transforms_per_step, step_end, transforms);
		*out_num_steps = uint32_t(step_end.size());
		if (out_steps != nullptr)
		{
			std::fill(out_steps, out_steps + num_tracks, 0u);
			uint32_t begin = 0;
			for (uint32_t step = 0; step < step_end.size(); ++step)
			{
				for (uint32_t k = begin; k < step_end[step]; ++k)
					out_steps[transforms[k]] = step + 1;
				begin = step_end[step];
			}
		}
		return ACLHIP_OK;
	});
}

extern "C" aclhip_status aclhip_set_clip_hierarchy(aclhip_context* context, aclhip_clip clip, const uint32_t* parent_indices, uint32_t num_tracks);

// aclhip_set_clip_hierarchy with the parent indices the blob carried (read at registration: parse_clip_metadata)
extern "C" aclhip_status aclhip_set_clip_hierarchy_from_metadata(aclhip_context* context, aclhip_clip clip)
{
	if (context == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	std::vector<uint32_t> parents;
	{
		std::shared_lock<std::shared_mutex> lock(context->mutex);
		if (clip >= context->clips.size() || !context->clips[clip].in_use)
			return fail(context, ACLHIP_ERROR_UNKNOWN_CLIP, "unknown clip handle %u", clip);
		if (context->clips[clip].metadata.has_parent_track_indices == 0)
			return fail(context, ACLHIP_ERROR_NO_METADATA, "clip %u was compressed without include_parent_track_indices: pass the hierarchy to aclhip_set_clip_hierarchy", clip);
		parents = context->clips[clip].metadata_parents;
	}
	return aclhip_set_clip_hierarchy(context, clip, parents.data(), uint32_t(parents.size()));
}

extern "C" aclhip_status aclhip_set_clip_hierarchy(aclhip_context* context, aclhip_clip clip, const uint32_t* parent_indices, uint32_t num_tracks)
{
	if (context == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	if (parent_indices == nullptr && num_tracks != 0)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null parent index list");

	return guarded(context, [&]() -> aclhip_status
	{
		std::lock_guard<std::shared_mutex> lock(context->mutex);
		if (clip >= context->clips.size() || !context->clips[clip].in_use)
			return fail(context, ACLHIP_ERROR_UNKNOWN_CLIP, "unknown clip handle %u", clip);
		host_clip& entry = context->clips[clip];
		if (entry.info.track_type != k_track_type_qvvf)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "clip %u is a scalar track list: no hierarchy", clip);
		if (entry.info.num_tracks != num_tracks)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%u parent indices for a clip of %u tracks", num_tracks, entry.info.num_tracks);
		if (num_tracks > 0xFFFFu)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%u transforms: the pose consumers end at about 3400", num_tracks);

		hierarchy_tree tree;
		uint32_t misplaced = 0;
		if (!build_hierarchy_tree(parent_indices, num_tracks, tree, misplaced))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "transform %u has parent %u: transforms must be sorted parent first", misplaced, parent_indices[misplaced]);
		std::vector<uint32_t> image;
		const uint32_t max_schedule_words = build_walk_schedule_image(tree, parent_indices, num_tracks, image);

		device_guard guard(context->device);

		// an identical hierarchy (another clip of the same skeleton) is already on the device?
		staged_hierarchy staged;
		size_t staging_used = 0;
		bool uploaded = stage_hierarchy(context, parent_indices, num_tracks, image, staging_used, staged);
		if (staged.d_image == nullptr)
			return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the hierarchy failed", image.size() * sizeof(uint32_t));
		uint32_t* d_hierarchy = staged.d_image;
		// launches in flight may still walk the hierarchy that is being replaced: it is retired, not freed (see retire())
		uploaded = uploaded && stage_upload(context, reinterpret_cast<uint8_t*>(context->d_clips + clip) + offsetof(device_clip, hierarchy), &d_hierarchy, sizeof(d_hierarchy), staging_used)
			&& finish_uploads(context);
		if (!uploaded)
		{
			drop_hierarchy(context, staged);
			return fail(context, ACLHIP_ERROR_DEVICE, "uploading the hierarchy failed");
		}
		keep_hierarchy(context, staged);
		if (entry.d_hierarchy != nullptr)
		{
			aclhip_context::retired_item item;
			item.hierarchy = entry.d_hierarchy;
			retire(context, std::move(item));
		}
		entry.d_hierarchy = d_hierarchy;
		const bool held_maximum = entry.hierarchy_words != 0 && entry.hierarchy_words == context->max_hierarchy_words;
		entry.hierarchy_words = max_schedule_words;
		context->max_hierarchy_words = std::max(context->max_hierarchy_words, max_schedule_words);
		if (held_maximum && max_schedule_words < context->max_hierarchy_words)
			recompute_launch_maxima(context);
		return ACLHIP_OK;
	});
}

namespace
{
	// The three entry points of the pose consumers (kernels_consumers.inl, kernels_skeleton.inl) share their leading arguments; the
	// skeleton space kernels take the mapping behind them, the masked ones the masking behind that, the additive ones the layering
	template<class... trailing_types>
	using pose_consumer_kernel = void (*)(const device_clip*, uint32_t, const uint32_t*, const float*, uint32_t, decode_params, consumer_params, uint8_t*, uint64_t, uint32_t, uint32_t, uint32_t, unsigned long long*, trailing_types...);

	template<class function_type>
	auto with_constant(bool value, function_type function)
	{
		return value ? function(std::true_type()) : function(std::false_type());
	}

	// rtm::qvv_mul's matrix route (kMirrored) is compiled in only where transforms are multiplied -- object space, or the relative format (a
	// base buffer, a second wave's image) -- and a caller's base buffer, of which the library knows nothing, always has it
	constexpr bool matrix_route_of(bool object_space, uint32_t base_kind, bool mirrored)
	{
		const bool multiplies_transforms = object_space || base_kind == k_consumer_base_buffer || base_kind == k_consumer_base_second_wave;
		return base_kind == k_consumer_base_buffer || (mirrored && multiplies_transforms);
	}

	// A launch's facts -> the instantiation of one of the entry points: instantiation_of(object space, kind of base, matrix route), each
	// an integral_constant. Only the combinations matrix_route_of can give are instantiated; a blend's base clip is never fused: no such
	// instantiation, a null pointer.
	template<class kernel_type, bool kBlend, class instantiation_type>
	kernel_type pose_consumer_kernel_of(bool object_space, uint32_t base_kind, bool mirrored, instantiation_type instantiation_of)
	{
		const bool matrix_route = matrix_route_of(object_space, base_kind, mirrored);
		return with_constant(object_space, [&](auto space) { return with_constant(matrix_route, [&](auto route)
		{
			const auto of_base = [&](auto base) -> kernel_type
			{
				if constexpr (matrix_route_of(decltype(space)::value, decltype(base)::value, decltype(route)::value) != decltype(route)::value || (kBlend && decltype(base)::value == k_consumer_base_fused))
					return nullptr;		// (never selected: not instantiated)
				else
					return instantiation_of(space, base, route);
			};
			switch (base_kind)
			{
			case k_consumer_base_none: return of_base(std::integral_constant<uint32_t, k_consumer_base_none>());
			case k_consumer_base_buffer: return of_base(std::integral_constant<uint32_t, k_consumer_base_buffer>());
			case k_consumer_base_second_wave: return of_base(std::integral_constant<uint32_t, k_consumer_base_second_wave>());
			default: return of_base(std::integral_constant<uint32_t, k_consumer_base_fused>());
			}
		}); });
	}

	// the same for the entry points that have blend as a template parameter of their own: instantiation_of takes it as a fourth constant
	template<class kernel_type, class instantiation_type>
	kernel_type pose_consumer_kernel_of(bool object_space, uint32_t base_kind, bool mirrored, bool blend, instantiation_type instantiation_of)
	{
		return with_constant(blend, [&](auto blended)
		{
			return pose_consumer_kernel_of<kernel_type, decltype(blended)::value>(object_space, base_kind, mirrored, [&](auto space, auto base, auto route) { return instantiation_of(space, base, route, blended); });
		});
	}

	// The instantiations of the three entry points for a launch without (no bounds_types) or with bounds (consumer_bounds_launch, the
	// kernels' last argument: aclhip_decompress_poses_batch_bounds). Bounds exist in object space only: no local space instantiation.
	template<class... bounds_types>
	struct pose_consumer_kernels
	{
		static constexpr bool with_bounds = sizeof...(bounds_types) != 0;
		using unmapped_type = pose_consumer_kernel<bounds_types...>;
		using skeleton_type = pose_consumer_kernel<skeleton_launch, bounds_types...>;
		using masked_type = pose_consumer_kernel<skeleton_launch, blend_mask_launch, bounds_types...>;
		using additive_type = pose_consumer_kernel<skeleton_launch, additive_strength_launch>;

		template<bool kObjectSpace, uint32_t kBase, bool kUnitScale, bool kMirrored, bool kBlend = false, bool kFast = false>
		static unmapped_type unmapped()
		{
			if constexpr (with_bounds && !kObjectSpace)
				return nullptr;
			else
				return decompress_poses_consumer_kernel<kObjectSpace, kBase, kUnitScale, kMirrored, kBlend, kFast, bounds_types...>;
		}
		template<bool kObjectSpace, uint32_t kBase, bool kMirrored, bool kBlend>
		static skeleton_type skeleton()
		{
			if constexpr (with_bounds && !kObjectSpace)
				return nullptr;
			else
				return decompress_poses_skeleton_kernel<kObjectSpace, kBase, kMirrored, kBlend, bounds_types...>;
		}
		template<bool kObjectSpace, uint32_t kBase, bool kMirrored>
		static masked_type masked()
		{
			if constexpr (with_bounds && !kObjectSpace)
				return nullptr;
			else
				return decompress_poses_masked_kernel<kObjectSpace, kBase, kMirrored, bounds_types...>;
		}
		// (aclhip_decompress_poses_batch_additive_weighted: additive formats only -- no instantiation without a base, none with bounds)
		template<bool kObjectSpace, uint32_t kBase, bool kMirrored, bool kBlend>
		static additive_type additive()
		{
			if constexpr (with_bounds || kBase == k_consumer_base_none)
				return nullptr;
			else
				return decompress_poses_additive_kernel<kObjectSpace, kBase, kMirrored, kBlend>;
		}
	};

	// The shape of a pose consumer launch (launch_consumers, launch_pose_rows): one wave per instance, the whole pose (its base, its
	// hierarchy) in LDS; as many instances per workgroup (a power of two, at most 8, 4 unless told otherwise: measured best) as leave room
	// for three workgroups per CU: the object space walk packs its lanes with instances of one workgroup.
	// what a workgroup may ask for on top of the kernel's static words (consumer_walk_slots, kernels_consumers.inl)
	constexpr size_t k_consumer_lds_bytes = 160 * 1024 - ((sizeof(consumer_walk_slots) + 127) / 128) * 128;
	struct consumer_launch_shape
	{
		uint32_t lds_quads_per_image;
		size_t lds_bytes_per_instance;
		uint32_t lds_schedule_words;
		uint32_t log2_instances_per_block;
		size_t lds_bytes;			// of a workgroup
		bool fits;					// lds_needed_bytes <= k_consumer_lds_bytes
		size_t lds_needed_bytes;	// of ONE instance and the schedule: what has to fit
	};

	// image_quads: the quads of an instance's image (exactly the transforms a pose row holds, or the largest registered clip has, not a quad
	// more: the kernel's "does the pose fit its image" test is also its "does the pose fit its row" test -- every quad is addressed on its
	// own: no granularity needed); max_hierarchy_words: the longest walk schedule registered (object space only, else 0 words are kept)
	consumer_launch_shape consumer_launch_shape_of(uint32_t image_quads, uint32_t batch_transforms, bool two_waves, bool object_space, uint32_t max_hierarchy_words)
	{
		consumer_launch_shape shape;
		shape.lds_quads_per_image = std::max<uint32_t>(image_quads, 1);
		// (measurement knob: ACLHIP_CONSUMER_LDS_PAD bytes between the instances' images -- the walk's lanes touch the same quad of all of a
		// workgroup's images at once, and images a multiple of 128 bytes apart put those on the same LDS banks)
		// 16 bytes: the four images of a workgroup then start on different banks (round 4: 88.8 -> 86.9 us, 90.6 -> 83.7 us with ACLHIP_CONSUMERS_FAST;
		// 32 the same, 64 less, 0 what rounds 2 and 3 measured)
		static const size_t lds_pad = []() { const char* value = lab_knob("ACLHIP_CONSUMER_LDS_PAD"); return value != nullptr ? size_t(std::atol(value)) & ~size_t(15) : size_t(16); }();
		shape.lds_bytes_per_instance = size_t(shape.lds_quads_per_image) * 16 * (two_waves ? 2 : 1) + lds_pad;
		// a walk schedule of T transforms: 2 words + a step end per step + a pair per transform with a parent, at most 2 + 2 T words
		shape.lds_schedule_words = object_space ? align_to_u32(std::max<uint32_t>(std::min<uint32_t>(max_hierarchy_words, 2 + 2 * batch_transforms + 3), 4), 4) : 0;
		const size_t lds_schedule_bytes = size_t(shape.lds_schedule_words) * sizeof(uint32_t);
		shape.lds_needed_bytes = shape.lds_bytes_per_instance + lds_schedule_bytes;
		shape.fits = shape.lds_needed_bytes <= k_consumer_lds_bytes;
		shape.log2_instances_per_block = 2;
		if (const char* forced = lab_knob("ACLHIP_CONSUMER_LOG2_INSTANCES"))
			shape.log2_instances_per_block = std::min<uint32_t>(uint32_t(forced[0] - '0'), 3);
		while (shape.log2_instances_per_block != 0 && (shape.lds_bytes_per_instance << shape.log2_instances_per_block) + lds_schedule_bytes > k_consumer_lds_bytes / 3)
			shape.log2_instances_per_block--;
		shape.lds_bytes = (shape.lds_bytes_per_instance << shape.log2_instances_per_block) + lds_schedule_bytes;
		return shape;
	}

	// The launch of a kernel of that shape, one wave per instance or two (launch_consumers and every launch of host_pose_buffers.inl):
	// above the default limit of dynamic LDS the kernel has to be told
	template<class kernel_type, class... argument_types>
	aclhip_status launch_consumer_kernel(aclhip_context* context, kernel_type kernel, const consumer_launch_shape& shape, uint32_t num_blocks, uint32_t waves_per_instance,
		hipStream_t stream, const argument_types&... arguments)
	{
		if (shape.lds_bytes > 64 * 1024 - 128)
			ACLHIP_CHECK_HIP(context, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(k_consumer_lds_bytes)));
		hipLaunchKernelGGL(kernel, dim3(num_blocks), dim3((waves_per_instance << shape.log2_instances_per_block) * k_wave_size), shape.lds_bytes, stream, arguments...);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}

	// What the skeleton space launches (_mapped, _masked, _bounds with a mapping) check of their mapping, and the launch argument made of it
	aclhip_status check_pose_mapping(aclhip_context* context, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping)
	{
		if (mapping->skeleton == 0 && mapping->instance_skeletons == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a pose mapping names a skeleton or a list of skeletons");
		if (mapping->map == 0 && mapping->instance_maps == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a pose mapping names a map or a list of maps");
		if (consumers->num_blend_clips > 1 && mapping->blend_maps == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a blend in skeleton space needs blend_maps");
		const bool base_is_clip = consumers->additive_format != ACLHIP_ADDITIVE_NONE && consumers->base_clips != nullptr;
		if (base_is_clip && mapping->base_maps == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "base clips in skeleton space need base_maps");
		return ACLHIP_OK;
	}

	// (the tables and their capacities are filled in by launch_consumers, under the registry lock: the same goes for the mask table below)
	skeleton_launch skeleton_launch_of(const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping)
	{
		const bool base_is_clip = consumers->additive_format != ACLHIP_ADDITIVE_NONE && consumers->base_clips != nullptr;
		skeleton_launch launch = {};
		launch.skeleton = mapping->skeleton;
		launch.map = mapping->map;
		launch.instance_skeletons = mapping->instance_skeletons;
		launch.instance_maps = mapping->instance_maps;
		launch.blend_maps = consumers->num_blend_clips > 1 ? mapping->blend_maps : nullptr;
		launch.base_maps = base_is_clip ? mapping->base_maps : nullptr;
		return launch;
	}

	// What the masked launches (_masked, _bounds with a masking) check of their masking, and the launch argument made of it
	aclhip_status check_blend_masking(aclhip_context* context, const aclhip_pose_consumers* consumers, const aclhip_blend_masking* masking)
	{
		if (masking->mode > ACLHIP_BLEND_LAYERED)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown blend mode %u", masking->mode);
		if (masking->reserved0 != 0 || masking->reserved[0] != 0 || masking->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of a blend masking are 0");
		if (masking->instance_masks == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a blend masking names a list of masks (entries may be 0)");
		if (consumers->num_blend_clips < 2)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "blend masks go with a blend: num_blend_clips is %u", consumers->num_blend_clips);
		return ACLHIP_OK;
	}

	blend_mask_launch blend_mask_launch_of(const aclhip_blend_masking* masking)
	{
		blend_mask_launch launch = {};
		launch.layered = masking->mode == ACLHIP_BLEND_LAYERED ? 1u : 0u;
		launch.instance_masks = masking->instance_masks;
		return launch;
	}

	// What every launch with bounds (_bounds, aclhip_transform_poses_batch) checks of the struct itself
	aclhip_status check_pose_bounds(aclhip_context* context, const aclhip_pose_bounds* bounds)
	{
		if (bounds->bounds == nullptr || (reinterpret_cast<uintptr_t>(bounds->bounds) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the bounds buffer must be set and 16 byte aligned");
		if (bounds->reserved[0] != 0 || bounds->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of pose bounds are 0");
		return ACLHIP_OK;
	}

	// What the additive launch checks of its layering
	aclhip_status check_additive_layering(aclhip_context* context, const aclhip_pose_consumers* consumers, const aclhip_additive_layering* layering)
	{
		if (layering->instance_weights == nullptr && layering->instance_masks == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive layering names instance_weights or instance_masks (without both it is aclhip_decompress_poses_batch_mapped)");
		if (layering->reserved[0] != 0 || layering->reserved[1] != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the reserved fields of an additive layering are 0");
		if (consumers->additive_format == ACLHIP_ADDITIVE_NONE)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive layering goes with an additive format: additive_format is NONE");
		return ACLHIP_OK;
	}

	// What a pose consumer launch takes on top of the plain one, each on its own switch: the device side of the caller's aclhip_pose_mapping,
	// aclhip_blend_masking, aclhip_pose_bounds and aclhip_additive_layering (launch_pose_consumers makes them)
	struct consumer_launch_extras
	{
		bool mapped = false, masked = false, bounded = false, layered = false;
		skeleton_launch mapping = {};
		blend_mask_launch masking = {};
		consumer_bounds_launch bounds = {};
		additive_strength_launch layering = {};
	};

	// `extras.mapped` (aclhip_decompress_poses_batch_mapped): skeleton space -- the launch is shaped by its rows alone (pose_stride_bytes / 48
	// slots), the skeleton kernels take the mapping as their trailing argument. `masked` (aclhip_decompress_poses_batch_masked, with a
	// mapping and a blend): the same launch through the masked kernels. `bounded` (aclhip_decompress_poses_batch_bounds, object space): the
	// same launch through the bounds instantiations, a box per instance on top of the rows -- or in their place, `poses` may then be null.
	// `layered` (aclhip_decompress_poses_batch_additive_weighted, with a mapping and an additive format, without masking and bounds): the
	// mapped launch through the additive kernels, a strength per (instance, slot) on the additive pose.
	aclhip_status launch_consumers(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
		const decode_params& params, const aclhip_pose_consumers& consumers, void* poses, uint64_t pose_stride_bytes, hipStream_t stream, consumer_launch_extras extras)
	{
		if (consumers.additive_format > ACLHIP_ADDITIVE_ADDITIVE1)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown additive format %u", consumers.additive_format);
		const bool has_base = consumers.additive_format != ACLHIP_ADDITIVE_NONE;
		const bool base_is_clip = has_base && consumers.base_clips != nullptr;
		if (base_is_clip && consumers.base_sample_times == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "base clips without base sample times");
		if (has_base && !base_is_clip && (consumers.base_poses == nullptr || (consumers.base_pose_stride_bytes & 15u) != 0 || (reinterpret_cast<uintptr_t>(consumers.base_poses) & 15u) != 0))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive format needs base clips or a 16 byte aligned base pose buffer");
		const bool blend = consumers.num_blend_clips > 1;
		if ((consumers.flags & ~ACLHIP_CONSUMERS_FAST) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown pose consumer flags 0x%x", consumers.flags);
		if (consumers.num_blend_clips > ACLHIP_MAX_BLEND_CLIPS)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a blend of %u clips: at most %u", consumers.num_blend_clips, ACLHIP_MAX_BLEND_CLIPS);
		if (blend && (consumers.blend_clips == nullptr || consumers.blend_sample_times == nullptr || consumers.blend_weights == nullptr))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a blend needs blend_clips, blend_sample_times and blend_weights");
		// a consumer needs every sub-track of the pose: the track_writer's own defaults (what the resolved pose image holds)
		if (params.standard_defaults == 0 || params.per_track_rounding != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose consumers take the track_writer's default sub-track modes, no per track rounding, normalization != always");

		std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
		if (extras.mapped)
		{
			if (context->skeletons.d_records == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no skeleton was ever registered with this context");
			if (context->track_maps.d_records == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no track map was ever registered with this context");
			extras.mapping.skeletons = context->skeletons.d_records;
			extras.mapping.num_skeletons = ACLHIP_MAX_SKELETONS;
			extras.mapping.maps = context->track_maps.d_records;
			extras.mapping.num_maps = ACLHIP_MAX_TRACK_MAPS;
		}
		// a masking or a layering with the context's mask table (no mask registered yet: a table of no records -- every handle but the null
		// handle is refused in the kernel)
		const auto with_mask_table = [&](auto& launch_argument)
		{
			launch_argument.masks = context->blend_masks.d_records;
			launch_argument.num_masks = context->blend_masks.d_records != nullptr ? ACLHIP_MAX_BLEND_MASKS : 0u;
		};
		if (extras.masked)
		{
			if (!extras.mapped || !blend)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "blend masks go with a blend in skeleton space");
			with_mask_table(extras.masking);
		}
		if (extras.layered)
		{
			if (!extras.mapped || !has_base || extras.masked || extras.bounded)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an additive layering goes with an additive format in skeleton space, without blend masks and bounds");
			with_mask_table(extras.layering);
		}
		note_launch_stream(context, stream);

		// No clip with a scale other than 1 registered, no base to combine with: every scale of every pose is 1, in local and in object
		// space -- the LDS images hold rotation | translation (32 of a transform's 48 bytes: half as many poses again per CU) and the
		// scales are written on the way out
		const bool unit_scale = !extras.mapped && !has_base && !blend && consumers.object_space != 0 && context->num_scaled_clips == 0 && path_knob("ACLHIP_CONSUMER_KEEP_SCALE") == nullptr;
		// (sized for the BATCH like every pose launch: no pose of it is larger than its row, pose_launch_shape_of in host_launch.inl --
		// one 3 500-bone asset in the registry does not take object space away from the 100-bone characters)
		// (skeleton space: the slots of a row, whatever clips are registered -- a clip may have more tracks than the skeleton has bones)
		const uint32_t batch_quads = extras.mapped ? uint32_t(std::min<uint64_t>(pose_stride_bytes / 48, 0xFFFFu)) * 3u : batch_pose_quads(context, ACLHIP_LAYOUT_QVV48, pose_stride_bytes);
		const uint32_t image_quads = unit_scale ? batch_quads / 3 * 2 : batch_quads;
		// additive0 / additive1 combine sub-track with sub-track: the base clip is decoded into the instance's image and the additive clip
		// onto it by one wave; the relative format (a qvv_mul) needs both poses whole: a second wave, a second image
		// (a blend accumulates its clips in the instance's image before anything else happens to it: its base clip gets a wave and an image of its own)
		const bool fused_base = base_is_clip && !blend && consumers.additive_format != ACLHIP_ADDITIVE_RELATIVE && lab_knob("ACLHIP_CONSUMER_TWO_IMAGES") == nullptr;
		const bool two_waves = base_is_clip && !fused_base;
		const consumer_launch_shape shape = consumer_launch_shape_of(image_quads, batch_quads / 3, two_waves, consumers.object_space != 0,
			extras.mapped ? context->max_skeleton_hierarchy_words : context->max_hierarchy_words);
		if (!shape.fits)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "poses of %u transforms (the pose stride, the largest registered clip): too large for the pose consumers (%zu bytes of LDS per instance)", batch_quads / 3, shape.lds_needed_bytes);
		const uint32_t instances_per_block = 1u << shape.log2_instances_per_block;
		const uint32_t num_blocks = (num_instances + instances_per_block - 1) / instances_per_block;

		consumer_params device_consumers;
		device_consumers.base_clip_ids = base_is_clip ? consumers.base_clips : nullptr;
		device_consumers.base_sample_times = base_is_clip ? consumers.base_sample_times : nullptr;
		device_consumers.base_poses = has_base && !base_is_clip ? static_cast<const uint8_t*>(consumers.base_poses) : nullptr;
		device_consumers.base_pose_stride_bytes = consumers.base_pose_stride_bytes;
		device_consumers.additive_format = consumers.additive_format;
		device_consumers.object_space = consumers.object_space != 0 ? 1 : 0;
		device_consumers.blend_clip_ids = blend ? consumers.blend_clips : nullptr;
		device_consumers.blend_sample_times = blend ? consumers.blend_sample_times : nullptr;
		device_consumers.blend_weights = blend ? consumers.blend_weights : nullptr;
		device_consumers.num_blend_clips = blend ? consumers.num_blend_clips : 0;

		// one instantiation per (object space, kind of base, rotation | translation images)
		const uint32_t base_kind = !has_base ? k_consumer_base_none : (!base_is_clip ? k_consumer_base_buffer : (fused_base ? k_consumer_base_fused : k_consumer_base_second_wave));
		// rtm::qvv_mul's matrix route (negative scales) is compiled into the launches that can meet one: a registered clip whose scale
		// sub-tracks may decode below zero, or a base the library knows nothing about (a caller's pose buffer)
		// (skeleton space: the reference pose fills slots -- like a clip whose scales registration has looked at)
		const bool mirrored = context->num_negative_scale_clips != 0 || (has_base && !base_is_clip) || (extras.mapped && context->num_negative_scale_skeletons != 0);
		const bool object_space = consumers.object_space != 0;
		// trailing: the mapping, the masking
		const auto launch = [&](auto kernel, const auto&... trailing) -> aclhip_status
		{
			if (kernel == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no pose consumer kernel for base kind %u", base_kind);
			return launch_consumer_kernel(context, kernel, shape, num_blocks, two_waves ? 2 : 1, stream,
				context->d_clips, context->d_clips_capacity, clips, sample_times, num_instances, params, device_consumers,
				static_cast<uint8_t*>(poses), pose_stride_bytes, shape.lds_quads_per_image, uint32_t(shape.lds_bytes_per_instance), shape.log2_instances_per_block | (shape.lds_schedule_words << 8), context->d_rejected, trailing...);
		};
		// ACLHIP_CONSUMERS_FAST: object space launches without a blend, in the hardware's 1 ulp arithmetic (include/aclhip.h)
		const bool fast = (consumers.flags & ACLHIP_CONSUMERS_FAST) != 0 && object_space && !blend;
		// trailing: nothing, or the bounds launch
		const auto launch_with = [&](const auto&... trailing) -> aclhip_status
		{
			using kernels = pose_consumer_kernels<std::decay_t<decltype(trailing)>...>;
			if constexpr (!kernels::with_bounds)		// (a layering comes without bounds: refused above)
				if (extras.layered)
					return launch(pose_consumer_kernel_of<typename kernels::additive_type>(object_space, base_kind, mirrored, blend, [](auto space, auto base, auto route, auto blended)
						{ return kernels::template additive<space(), base(), route(), blended()>(); }), extras.mapping, extras.layering);
			if (extras.masked)
				return launch(pose_consumer_kernel_of<typename kernels::masked_type, true>(object_space, base_kind, mirrored, [](auto space, auto base, auto route)
					{ return kernels::template masked<space(), base(), route()>(); }), extras.mapping, extras.masking, trailing...);
			if (extras.mapped)
				return launch(pose_consumer_kernel_of<typename kernels::skeleton_type>(object_space, base_kind, mirrored, blend, [](auto space, auto base, auto route, auto blended)
					{ return kernels::template skeleton<space(), base(), route(), blended()>(); }), extras.mapping, trailing...);
			// one instantiation per (object space, kind of base, matrix route); rotation | translation images: object space without a base only
			if (unit_scale)
				return launch(fast ? kernels::template unmapped<true, k_consumer_base_none, true, false, false, true>() : kernels::template unmapped<true, k_consumer_base_none, true, false>(), trailing...);
			if (blend)
				return launch(pose_consumer_kernel_of<typename kernels::unmapped_type, true>(object_space, base_kind, mirrored, [](auto space, auto base, auto route)
					{ return kernels::template unmapped<space(), base(), false, route(), true>(); }), trailing...);
			if (fast)		// (object space, see above)
				return launch(pose_consumer_kernel_of<typename kernels::unmapped_type, false>(true, base_kind, mirrored, [](auto, auto base, auto route)
					{ return kernels::template unmapped<true, base(), false, route(), false, true>(); }), trailing...);
			return launch(pose_consumer_kernel_of<typename kernels::unmapped_type, false>(object_space, base_kind, mirrored, [](auto space, auto base, auto route)
				{ return kernels::template unmapped<space(), base(), false, route()>(); }), trailing...);
		};
		return extras.bounded ? launch_with(extras.bounds) : launch_with();
	}

	// The caller's side of consumer_launch_extras: the optional structs of the pose launch entry points, null where an entry point has none
	struct pose_launch_structs
	{
		const aclhip_pose_mapping* mapping;
		const aclhip_blend_masking* masking;
		const aclhip_pose_bounds* bounds;
		const aclhip_additive_layering* layering;
	};

	// The one front of the five pose launch entry points (aclhip_decompress_poses_batch, _mapped, _masked, _bounds, _additive_weighted): each
	// says which of the four structs it requires and calls this. The argument checks that need no device come first and leave a message,
	// with or without a context -- the structs, the lists and the pose buffer (null with bounds: the boxes alone), the null context last.
	aclhip_status launch_pose_consumers(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
		const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const pose_launch_structs& structs, void* poses, uint64_t pose_stride_bytes, void* stream)
	{
		if (consumers == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null consumers");
		aclhip_status status = structs.bounds != nullptr ? check_pose_bounds(context, structs.bounds) : ACLHIP_OK;
		if (status == ACLHIP_OK && structs.bounds != nullptr && consumers->object_space == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose bounds are taken in object space: a local space translation is not a position");
		if (status == ACLHIP_OK && structs.masking != nullptr)
			status = structs.mapping != nullptr ? check_blend_masking(context, consumers, structs.masking) : fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "blend masks go with a pose mapping");
		if (status == ACLHIP_OK && structs.layering != nullptr)
			status = check_additive_layering(context, consumers, structs.layering);
		if (status == ACLHIP_OK && structs.mapping != nullptr)
			status = check_pose_mapping(context, consumers, structs.mapping);
		if (status == ACLHIP_OK)
			status = check_batch_arguments(context, clips, sample_times, num_instances, poses, pose_stride_bytes, structs.bounds != nullptr);
		if (status != ACLHIP_OK || num_instances == 0)
			return status;

		decode_params device_params;
		status = resolve_params(context, params, device_params);
		if (status != ACLHIP_OK)
			return status;

		consumer_launch_extras extras;
		extras.mapped = structs.mapping != nullptr;
		if (extras.mapped)
			extras.mapping = skeleton_launch_of(consumers, structs.mapping);
		extras.masked = structs.masking != nullptr;
		if (extras.masked)
			extras.masking = blend_mask_launch_of(structs.masking);
		extras.bounded = structs.bounds != nullptr;
		if (extras.bounded)
			extras.bounds = { static_cast<uint8_t*>(structs.bounds->bounds), structs.bounds->bone_flags };
		extras.layered = structs.layering != nullptr;
		if (extras.layered)
		{
			extras.layering.instance_weights = structs.layering->instance_weights;
			extras.layering.instance_masks = structs.layering->instance_masks;
		}

		device_guard guard(context->device);
		return launch_consumers(context, clips, sample_times, num_instances, device_params, *consumers, poses, pose_stride_bytes, static_cast<hipStream_t>(stream), extras);
	}
}

extern "C" aclhip_status aclhip_decompress_poses_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	return launch_pose_consumers(context, clips, sample_times, num_instances, params, consumers, {}, poses, pose_stride_bytes, stream);
}

namespace
{
	// Host pointer convenience path: upload, launch, download, synchronously
	aclhip_status decompress_host(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* track_indices, uint32_t num_instances,
		const aclhip_decompress_params* params, uint32_t default_values_count, void* out, uint64_t out_stride_bytes, uint64_t out_row_bytes,
		const aclhip_pose_consumers* consumers = nullptr, const aclhip_output_desc* output = nullptr)
	{
		if (context == nullptr)
			return ACLHIP_ERROR_INVALID_ARGUMENT;
		if (num_instances == 0)
			return ACLHIP_OK;
		if (clips == nullptr || sample_times == nullptr || out == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null instance list or output buffer");
		const uint32_t bytes_per_track = output != nullptr ? aclhip_layout_bytes_per_track(output->layout) : 48u;
		if (bytes_per_track == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown pose layout %u", output->layout);

		aclhip_decompress_params local;
		if (params != nullptr) local = *params; else aclhip_default_params(&local);

		device_guard guard(context->device);

		uint32_t max_tracks = 0;
		{
			std::lock_guard<std::shared_mutex> lock(context->mutex);
			for (uint32_t i = 0; i < num_instances; ++i)
				if (clips[i] < context->clips.size() && context->clips[clips[i]].in_use)
					max_tracks = std::max(max_tracks, context->clips[clips[i]].info.num_tracks);
		}

		const bool single_track = track_indices != nullptr;
		const uint64_t device_stride = single_track ? 48 : std::max<uint64_t>((uint64_t(max_tracks) * bytes_per_track + 15) & ~uint64_t(15), 16);
		if (!single_track && out_row_bytes == 0)
			out_row_bytes = uint64_t(max_tracks) * bytes_per_track;

		// (the host convenience calls are synchronous by contract and stage through temporary device buffers on the default stream;
		// callers that must not disturb work in flight use the device pointer entry points)
		hipStream_t work_stream = nullptr;
		std::vector<void*> allocations;
		auto release = [&]() { for (void* p : allocations) (void)hipFree(p); };
		auto upload = [&](const void* host, size_t bytes, void** out_device) -> bool
		{
			void* d = nullptr;
			if (hipMalloc(&d, std::max<size_t>(bytes, 16)) != hipSuccess)
				return false;
			allocations.push_back(d);
			if (host != nullptr && hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess)
				return false;
			*out_device = d;
			return true;
		};

		void* d_clip_ids = nullptr; void* d_times = nullptr; void* d_tracks = nullptr; void* d_out = nullptr;
		void* d_defaults = nullptr; void* d_track_policies = nullptr; void* d_instance_policies = nullptr;
		bool ok = upload(clips, sizeof(uint32_t) * num_instances, &d_clip_ids) && upload(sample_times, sizeof(float) * num_instances, &d_times);
		if (ok && single_track)
			ok = upload(track_indices, sizeof(uint32_t) * num_instances, &d_tracks);
		ok = ok && upload(nullptr, device_stride * num_instances, &d_out);
		aclhip_output_desc local_output = {};
		if (output != nullptr)
		{
			// (the same refusals apply_output_desc makes for the device entry points, BEFORE anything is uploaded: a descriptor with one of
			// the two mask arrays used to be decoded here without masks)
			if ((output->instance_masks != nullptr) != (output->mask_table != nullptr))
			{
				release();
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "instance_masks and mask_table come together");
			}
			if (output->instance_masks != nullptr && output->mask_stride == 0)
			{
				release();
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "mask_stride: the bytes of one mask of mask_table (at least the tracks of the largest clip of the batch)");
			}
			local_output = *output;
			void* d_rows = nullptr;
			if (ok && output->rows != nullptr)
				ok = upload(output->rows, sizeof(uint32_t) * num_instances, &d_rows);
			local_output.rows = static_cast<const uint32_t*>(d_rows);
			void* d_skip_tracks = nullptr;
			if (ok && output->skip_tracks != nullptr)
				ok = upload(output->skip_tracks, std::max<uint32_t>(max_tracks, 1), &d_skip_tracks);
			local_output.skip_tracks = static_cast<const uint8_t*>(d_skip_tracks);
			// per instance writer decisions: the masks the instances name (as many as the largest index says), their track counts
			void* d_instance_masks = nullptr; void* d_mask_table = nullptr; void* d_track_counts = nullptr;
			if (ok && output->instance_masks != nullptr && output->mask_table != nullptr)
			{
				uint32_t num_masks = 0;
				for (uint32_t i = 0; i < num_instances; ++i)
					num_masks = std::max<uint32_t>(num_masks, uint32_t(output->instance_masks[i]) + 1);
				ok = upload(output->instance_masks, num_instances, &d_instance_masks) && upload(output->mask_table, size_t(num_masks) * output->mask_stride, &d_mask_table);
			}
			if (ok && output->instance_track_counts != nullptr)
				ok = upload(output->instance_track_counts, sizeof(uint32_t) * num_instances, &d_track_counts);
			local_output.instance_masks = output->instance_masks != nullptr ? static_cast<const uint8_t*>(d_instance_masks) : nullptr;
			local_output.mask_table = output->mask_table != nullptr ? static_cast<const uint8_t*>(d_mask_table) : nullptr;
			local_output.instance_track_counts = static_cast<const uint32_t*>(d_track_counts);
		}
		if (ok && local.default_values != nullptr)
			ok = upload(local.default_values, size_t(std::max<uint32_t>(default_values_count, 1)) * 48, &d_defaults);
		if (ok && local.track_rounding_policies != nullptr)
			ok = upload(local.track_rounding_policies, std::max<uint32_t>(max_tracks, 1), &d_track_policies);
		if (ok && local.instance_rounding_policies != nullptr)
			ok = upload(local.instance_rounding_policies, num_instances, &d_instance_policies);
		void* d_instance_looping = nullptr;
		if (ok && local.instance_looping_policies != nullptr)
			ok = upload(local.instance_looping_policies, num_instances, &d_instance_looping);
		// per instance writers' track rounding tables: as many tables as the largest index names
		void* d_rounding_table = nullptr; void* d_rounding_tables_of = nullptr;
		if (ok && local.track_rounding_table != nullptr && local.instance_rounding_tables != nullptr)
		{
			uint32_t num_tables = 0;
			for (uint32_t i = 0; i < num_instances; ++i)
				num_tables = std::max<uint32_t>(num_tables, uint32_t(local.instance_rounding_tables[i]) + 1);
			ok = upload(local.instance_rounding_tables, num_instances, &d_rounding_tables_of) && upload(local.track_rounding_table, size_t(num_tables) * local.track_rounding_stride, &d_rounding_table);
		}

		aclhip_pose_consumers local_consumers = {};
		if (consumers != nullptr)
		{
			local_consumers = *consumers;
			void* d_base_clips = nullptr; void* d_base_times = nullptr; void* d_base_poses = nullptr;
			if (ok && consumers->base_clips != nullptr)
				ok = upload(consumers->base_clips, sizeof(uint32_t) * num_instances, &d_base_clips);
			if (ok && consumers->base_sample_times != nullptr)
				ok = upload(consumers->base_sample_times, sizeof(float) * num_instances, &d_base_times);
			if (ok && consumers->base_poses != nullptr && consumers->base_clips == nullptr && consumers->additive_format != ACLHIP_ADDITIVE_NONE)
			{
				if (consumers->base_pose_stride_bytes < uint64_t(max_tracks) * 48)
				{
					release();
					return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "base pose stride %llu is smaller than a pose of %u transforms", (unsigned long long)consumers->base_pose_stride_bytes, max_tracks);
				}
				ok = upload(consumers->base_poses, size_t(consumers->base_pose_stride_bytes) * num_instances, &d_base_poses);
			}
			local_consumers.base_clips = static_cast<const aclhip_clip*>(d_base_clips);
			local_consumers.base_sample_times = static_cast<const float*>(d_base_times);
			local_consumers.base_poses = d_base_poses;
			if (consumers->num_blend_clips > 1 && consumers->num_blend_clips <= ACLHIP_MAX_BLEND_CLIPS
				&& consumers->blend_clips != nullptr && consumers->blend_sample_times != nullptr && consumers->blend_weights != nullptr)
			{
				const size_t others = size_t(num_instances) * (consumers->num_blend_clips - 1);
				void* d_blend_clips = nullptr; void* d_blend_times = nullptr; void* d_blend_weights = nullptr;
				ok = ok && upload(consumers->blend_clips, sizeof(uint32_t) * others, &d_blend_clips) && upload(consumers->blend_sample_times, sizeof(float) * others, &d_blend_times)
					&& upload(consumers->blend_weights, sizeof(float) * size_t(num_instances) * consumers->num_blend_clips, &d_blend_weights);
				local_consumers.blend_clips = static_cast<const aclhip_clip*>(d_blend_clips);
				local_consumers.blend_sample_times = static_cast<const float*>(d_blend_times);
				local_consumers.blend_weights = static_cast<const float*>(d_blend_weights);
			}
		}
		if (!ok)
		{
			release();
			return fail(context, ACLHIP_ERROR_DEVICE, "staging the batch on the device failed");
		}

		// Bytes the decode does not write (skipped defaults, tracks beyond a smaller clip's count, rejected instances) must keep
		// what the caller had there: round trip the caller's buffer
		{
			const hipError_t copy_status = hipMemcpy2D(d_out, device_stride, out, out_stride_bytes, std::min<uint64_t>(out_row_bytes, device_stride), num_instances, hipMemcpyHostToDevice);
			if (copy_status != hipSuccess)
			{
				release();
				return fail(context, ACLHIP_ERROR_DEVICE, "uploading the caller's pose buffer failed: %s", hipGetErrorString(copy_status));
			}
		}

		local.default_values = static_cast<const float*>(d_defaults);
		local.track_rounding_policies = static_cast<const uint8_t*>(d_track_policies);
		local.instance_rounding_policies = static_cast<const uint8_t*>(d_instance_policies);
		local.instance_looping_policies = static_cast<const uint8_t*>(d_instance_looping);
		if (local.track_rounding_table != nullptr && local.instance_rounding_tables != nullptr)
		{
			local.track_rounding_table = static_cast<const uint8_t*>(d_rounding_table);
			local.instance_rounding_tables = static_cast<const uint8_t*>(d_rounding_tables_of);
		}

		aclhip_status status;
		if (single_track)
			status = aclhip_decompress_track_batch(context, static_cast<const aclhip_clip*>(d_clip_ids), static_cast<const float*>(d_times), static_cast<const uint32_t*>(d_tracks), num_instances, &local, d_out, work_stream);
		else if (consumers != nullptr)
			status = aclhip_decompress_poses_batch(context, static_cast<const aclhip_clip*>(d_clip_ids), static_cast<const float*>(d_times), num_instances, &local, &local_consumers, d_out, device_stride, work_stream);
		else
			status = aclhip_decompress_tracks_batch_out(context, static_cast<const aclhip_clip*>(d_clip_ids), static_cast<const float*>(d_times), num_instances, &local,
				output != nullptr ? &local_output : nullptr, d_out, device_stride, work_stream);

		if (status == ACLHIP_OK)
		{
			hipError_t copy_status = hipStreamSynchronize(work_stream);
			if (copy_status == hipSuccess)
				copy_status = hipMemcpy2D(out, out_stride_bytes, d_out, device_stride, std::min<uint64_t>(out_row_bytes, device_stride), num_instances, hipMemcpyDeviceToHost);
			if (copy_status != hipSuccess)
				status = fail(context, ACLHIP_ERROR_DEVICE, "downloading the poses failed: %s", hipGetErrorString(copy_status));
		}

		release();
		return status;
	}
}

extern "C" aclhip_status aclhip_decompress_tracks_host(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, uint32_t default_values_count, void* poses, uint64_t pose_stride_bytes)
{
	return decompress_host(context, clips, sample_times, nullptr, num_instances, params, default_values_count, poses, pose_stride_bytes, 0);
}

extern "C" aclhip_status aclhip_decompress_tracks_host_out(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, uint32_t default_values_count, const aclhip_output_desc* output, void* poses, uint64_t pose_stride_bytes)
{
	return decompress_host(context, clips, sample_times, nullptr, num_instances, params, default_values_count, poses, pose_stride_bytes, 0, nullptr, output);
}

extern "C" aclhip_status aclhip_decompress_poses_host(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, void* poses, uint64_t pose_stride_bytes)
{
	if (consumers == nullptr)
		return context != nullptr ? fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null consumers") : ACLHIP_ERROR_INVALID_ARGUMENT;
	if (params != nullptr && (params->default_values != nullptr || params->track_rounding_policies != nullptr || params->track_rounding_table != nullptr))
		return context != nullptr ? fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "pose consumers take the track_writer's default sub-track modes, no per track rounding") : ACLHIP_ERROR_INVALID_ARGUMENT;
	return decompress_host(context, clips, sample_times, nullptr, num_instances, params, 0, poses, pose_stride_bytes, 0, consumers);
}

extern "C" aclhip_status aclhip_decompress_track_host(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* track_indices,
	uint32_t num_instances, const aclhip_decompress_params* params, uint32_t default_values_count, void* transforms)
{
	if (track_indices == nullptr)
		return context != nullptr ? fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null track index list") : ACLHIP_ERROR_INVALID_ARGUMENT;
	return decompress_host(context, clips, sample_times, track_indices, num_instances, params, default_values_count, transforms, 48, 48);
}

#if defined(ACLHIP_EXP_PHASE_TIMES)
// measurement aid, see kernels_consumers.inl
extern "C" int aclhip_debug_read_phase_times(unsigned long long* out, uint32_t count)
{
	return int(hipMemcpyFromSymbol(out, HIP_SYMBOL(aclhip::phase_times), size_t(count) * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost));
}
#endif
