// host_skeletons.inl -- part of aclhip.hip (one translation unit; included there, in this order, not compiled on its own).
// Host side: skeletons (what the slot space of a set of track maps means) and the pose consumers' launch in skeleton space.

namespace
{
	// What registration checks; the message names the first offending bone. `out_tree`: the hierarchy, when there is one.
	bool check_skeleton(const uint32_t* parent_indices, const void* reference_pose, uint32_t num_bones, aclhip_skeleton_info& info, hierarchy_tree* out_tree,
		char* message, size_t capacity)
	{
		const auto say = [&](const char* format, uint32_t a, uint32_t b)
		{
			if (message != nullptr && capacity != 0)
				std::snprintf(message, capacity, format, a, b);
			return false;
		};
		if (message != nullptr && capacity != 0)
			message[0] = '\0';
		std::memset(&info, 0, sizeof(info));
		if (reference_pose == nullptr)
			return say("null reference pose", 0, 0);
		if (num_bones == 0)
			return say("a skeleton of %u bones", num_bones, 0);
		if (num_bones > 0xFFFFu)
			return say("%u bones: a skeleton holds at most %u", num_bones, 0xFFFFu);

		info.num_bones = num_bones;
		if (parent_indices != nullptr)
		{
			hierarchy_tree tree;
			uint32_t misplaced = 0;
			if (!build_hierarchy_tree(parent_indices, num_bones, tree, misplaced))
				return say("bone %u has parent %u: bones must be sorted parent first", misplaced, parent_indices[misplaced]);
			info.has_hierarchy = 1;
			for (uint32_t bone = 0; bone < num_bones; ++bone)
				if (tree.is_root[bone])
				{
					info.num_roots++;
					info.depth = std::max(info.depth, tree.height[bone]);
				}
			std::vector<uint32_t> step_end, transforms;
			schedule_hierarchy_walk(tree, num_bones, 16, step_end, transforms);
			info.walk_steps = uint32_t(step_end.size());
			if (out_tree != nullptr)
				*out_tree = std::move(tree);
		}

		const float* values = static_cast<const float*>(reference_pose);
		for (uint32_t bone = 0; bone < num_bones; ++bone)
		{
			for (uint32_t component = 0; component < 12; ++component)
			{
				const bool is_pad = component == 7 || component == 11;
				if (!is_pad && !std::isfinite(values[size_t(bone) * 12 + component]))
					return say("bone %u: component %u of its reference transform is not finite", bone, component);
			}
			for (uint32_t component = 8; component < 11; ++component)
				if (values[size_t(bone) * 12 + component] < 0.0f)
					info.has_negative_scale = 1;
		}
		return true;
	}
}

extern "C" aclhip_status aclhip_check_skeleton(const uint32_t* parent_indices, const void* reference_pose, uint32_t num_bones, aclhip_skeleton_info* out_info,
	char* message, uint32_t message_capacity)
{
	return guarded(static_cast<aclhip_context*>(nullptr), [&]() -> aclhip_status
	{
		aclhip_skeleton_info info;
		const bool valid = check_skeleton(parent_indices, reference_pose, num_bones, info, nullptr, message, message_capacity);
		if (valid && out_info != nullptr)
			*out_info = info;
		return valid ? ACLHIP_OK : ACLHIP_ERROR_INVALID_ARGUMENT;
	});
}

extern "C" aclhip_status aclhip_register_skeleton(aclhip_context* context, const uint32_t* parent_indices, const void* reference_pose, uint32_t num_bones, aclhip_skeleton* out_skeleton)
{
	if (context == nullptr || out_skeleton == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	*out_skeleton = 0;
	return guarded(context, [&]() -> aclhip_status
	{
		// (everything that needs no device first: a refused skeleton makes no HIP call)
		aclhip_skeleton_info info;
		hierarchy_tree tree;
		char message[256];
		if (!check_skeleton(parent_indices, reference_pose, num_bones, info, &tree, message, sizeof(message)))
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s", message);

		// the reference pose as an image of quads: the pads of translations and scales are 0, like every pose the decode writes
		std::vector<float> pose(static_cast<const float*>(reference_pose), static_cast<const float*>(reference_pose) + size_t(num_bones) * 12);
		bool short_exact_math = true;
		for (uint32_t bone = 0; bone < num_bones; ++bone)
		{
			float* record = pose.data() + size_t(bone) * 12;
			record[7] = record[11] = 0.0f;
			const double length_squared = double(record[0]) * record[0] + double(record[1]) * record[1] + double(record[2]) * record[2] + double(record[3]) * record[3];
			short_exact_math = short_exact_math && length_squared >= 0.25 && length_squared <= 4.0;
		}
		std::vector<uint32_t> schedule_image;
		uint32_t schedule_words = 0;
		if (parent_indices != nullptr)
			schedule_words = build_walk_schedule_image(tree, parent_indices, num_bones, schedule_image);

		std::lock_guard<std::shared_mutex> lock(context->mutex);
		device_guard guard(context->device);
		collect_retired(context, false);

		if (context->d_skeletons == nullptr)
		{
			// once: the table never moves and never grows (a cleared record is an unknown skeleton)
			device_skeleton* table = nullptr;
			ACLHIP_CHECK_HIP(context, hipMalloc(reinterpret_cast<void**>(&table), sizeof(device_skeleton) * ACLHIP_MAX_SKELETONS));
			hipError_t zeroed = hipMemsetAsync(table, 0, sizeof(device_skeleton) * ACLHIP_MAX_SKELETONS, context->copy_stream);
			if (zeroed == hipSuccess)
				zeroed = hipStreamSynchronize(context->copy_stream);
			if (zeroed != hipSuccess)
			{
				(void)hipFree(table);
				ACLHIP_CHECK_HIP(context, zeroed);
			}
			context->d_skeletons = table;
			context->skeletons.resize(1);		// handle 0: none
		}

		uint32_t slot;
		if (!context->free_skeleton_slots.empty())
		{
			slot = context->free_skeleton_slots.back();
			context->free_skeleton_slots.pop_back();
		}
		else
		{
			if (context->skeletons.size() >= ACLHIP_MAX_SKELETONS)
				return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "the skeleton table holds %u skeletons", ACLHIP_MAX_SKELETONS - 1);
			slot = uint32_t(context->skeletons.size());
			context->skeletons.emplace_back();
		}
		const auto give_back = [&]() { context->free_skeleton_slots.push_back(slot); };

		const size_t pose_bytes = pose.size() * sizeof(float);
		uint8_t* d_pose = allocate_clip_memory(context, pose_bytes);
		if (d_pose == nullptr)
		{
			give_back();
			return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the reference pose failed", pose_bytes);
		}
		size_t staging_used = 0;
		staged_hierarchy staged;
		bool uploaded = true;
		if (parent_indices != nullptr)
		{
			// the walk schedule image exactly as a clip's: shared with every clip and skeleton of the same hierarchy
			uploaded = stage_hierarchy(context, parent_indices, num_bones, schedule_image, staging_used, staged);
			if (staged.d_image == nullptr)
			{
				free_clip_memory(context, d_pose);
				give_back();
				return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the hierarchy failed", schedule_image.size() * sizeof(uint32_t));
			}
		}
		device_skeleton record;
		std::memset(&record, 0, sizeof(record));
		record.hierarchy = staged.d_image;
		record.reference_pose = reinterpret_cast<const f32x4*>(d_pose);
		record.num_bones = num_bones;
		record.flags = (info.has_negative_scale != 0 ? k_skeleton_negative_scale : 0u) | (short_exact_math ? k_skeleton_short_exact_math : 0u);
		// the images first, the record that publishes them behind them (one stream: in order)
		uploaded = uploaded && stage_upload(context, d_pose, pose.data(), pose_bytes, staging_used)
			&& stage_upload(context, context->d_skeletons + slot, &record, sizeof(record), staging_used)
			&& finish_uploads(context);
		if (!uploaded)
		{
			drop_hierarchy(context, staged);
			free_clip_memory(context, d_pose);
			give_back();
			return fail(context, ACLHIP_ERROR_DEVICE, "uploading the skeleton failed");
		}
		if (staged.d_image != nullptr)
			keep_hierarchy(context, staged);
		aclhip_context::skeleton_entry& entry = context->skeletons[slot];
		entry.in_use = true;
		entry.info = info;
		entry.device_memory = d_pose;
		entry.d_hierarchy = record.hierarchy != nullptr ? const_cast<uint32_t*>(record.hierarchy) : nullptr;
		entry.negative_scale = info.has_negative_scale != 0;
		context->num_negative_scale_skeletons += entry.negative_scale ? 1u : 0u;
		context->max_skeleton_hierarchy_words = std::max(context->max_skeleton_hierarchy_words, schedule_words);
		*out_skeleton = slot;
		return ACLHIP_OK;
	});
}

extern "C" aclhip_status aclhip_unregister_skeleton(aclhip_context* context, aclhip_skeleton skeleton)
{
	if (context == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;

	std::lock_guard<std::shared_mutex> lock(context->mutex);
	if (skeleton == 0 || skeleton >= context->skeletons.size() || !context->skeletons[skeleton].in_use)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown skeleton handle %u", skeleton);

	device_guard guard(context->device);
	collect_retired(context, false);
	// stream ordered, nobody waits (aclhip_unregister_track_map): the record is cleared behind the launches already enqueued, the
	// reference pose, the walk schedule (when this was its last user) and the handle are recycled once both have happened
	aclhip_context::retired_item item;
	item.clip_memory = context->skeletons[skeleton].device_memory;
	item.hierarchy = context->skeletons[skeleton].d_hierarchy;
	item.skeleton_slot = skeleton;
	retire(context, std::move(item), context->d_skeletons + skeleton, sizeof(device_skeleton));
	context->num_negative_scale_skeletons -= context->skeletons[skeleton].negative_scale ? 1u : 0u;
	context->skeletons[skeleton] = aclhip_context::skeleton_entry();
	return ACLHIP_OK;
}

extern "C" aclhip_status aclhip_get_skeleton_info(const aclhip_context* context, aclhip_skeleton skeleton, aclhip_skeleton_info* out_info)
{
	if (context == nullptr || out_info == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	aclhip_context* mutable_context = const_cast<aclhip_context*>(context);
	std::shared_lock<std::shared_mutex> lock(mutable_context->mutex);
	if (skeleton == 0 || skeleton >= context->skeletons.size() || !context->skeletons[skeleton].in_use)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown skeleton handle %u", skeleton);
	*out_info = context->skeletons[skeleton].info;
	return ACLHIP_OK;
}

namespace
{
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

	// (the tables and their capacities are filled in by launch_consumers, under the registry lock)
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
}

extern "C" aclhip_status aclhip_decompress_poses_batch_mapped(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	aclhip_status status = check_batch_arguments(context, clips, sample_times, num_instances, poses, pose_stride_bytes);
	if (status != ACLHIP_OK)
		return status;
	if (consumers == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null consumers");
	if (mapping == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose mapping");
	status = check_pose_mapping(context, consumers, mapping);
	if (status != ACLHIP_OK)
		return status;
	if (num_instances == 0)
		return ACLHIP_OK;

	decode_params device_params;
	status = resolve_params(context, params, device_params);
	if (status != ACLHIP_OK)
		return status;

	const skeleton_launch launch = skeleton_launch_of(consumers, mapping);

	device_guard guard(context->device);
	return launch_consumers(context, clips, sample_times, num_instances, device_params, *consumers, poses, pose_stride_bytes, static_cast<hipStream_t>(stream), &launch);
}
