// host_skeletons.inl -- part of aclhip.hip (one translation unit; included there, in this order, not compiled on its own).
// Host side: skeletons (what the slot space of a set of track maps means) -- what registration checks, the record, its reference pose and
// its share of a walk schedule image; the handles are a handle_table's (host_context.inl) -- and the pose consumers' launch in skeleton space.

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

		uint32_t slot;
		if (const aclhip_status status = take_handle(context, context->skeletons, slot); status != ACLHIP_OK)
			return status;

		const size_t pose_bytes = pose.size() * sizeof(float);
		uint8_t* d_pose = allocate_clip_memory(context, pose_bytes);
		if (d_pose == nullptr)
		{
			context->skeletons.give_back(slot);
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
				context->skeletons.give_back(slot);
				return fail(context, ACLHIP_ERROR_OUT_OF_MEMORY, "allocating %zu bytes for the hierarchy failed", schedule_image.size() * sizeof(uint32_t));
			}
		}
		device_skeleton record;
		std::memset(&record, 0, sizeof(record));
		record.hierarchy = staged.d_image;
		record.reference_pose = reinterpret_cast<const f32x4*>(d_pose);
		record.num_bones = num_bones;
		record.flags = (info.has_negative_scale != 0 ? k_skeleton_negative_scale : 0u) | (short_exact_math ? k_skeleton_short_exact_math : 0u);
		// the images first, the record that publishes them behind them
		uploaded = uploaded && stage_upload(context, d_pose, pose.data(), pose_bytes, staging_used)
			&& publish_handle(context, context->skeletons, slot, record, staging_used, info, d_pose);
		if (!uploaded)
		{
			drop_hierarchy(context, staged);
			free_clip_memory(context, d_pose);
			context->skeletons.give_back(slot);
			return fail(context, ACLHIP_ERROR_DEVICE, "uploading the skeleton failed");
		}
		if (staged.d_image != nullptr)
			keep_hierarchy(context, staged);
		auto& entry = context->skeletons.entries[slot];
		entry.d_hierarchy = staged.d_image;
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
	// on top of the reference pose and the handle: its share of the walk schedule (freed when this was the image's last user)
	return unregister_handle(context, context->skeletons, skeleton, [&](const auto& entry, aclhip_context::retired_item& item)
	{
		item.hierarchy = entry.d_hierarchy;
		context->num_negative_scale_skeletons -= entry.negative_scale ? 1u : 0u;
	});
}

extern "C" aclhip_status aclhip_get_skeleton_info(const aclhip_context* context, aclhip_skeleton skeleton, aclhip_skeleton_info* out_info)
{
	if (context == nullptr || out_info == nullptr)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return get_handle_info(context, context->skeletons, skeleton, out_info);
}

extern "C" aclhip_status aclhip_decompress_poses_batch_mapped(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, uint32_t num_instances,
	const aclhip_decompress_params* params, const aclhip_pose_consumers* consumers, const aclhip_pose_mapping* mapping, void* poses, uint64_t pose_stride_bytes, void* stream)
{
	if (mapping == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose mapping");
	return launch_pose_consumers(context, clips, sample_times, num_instances, params, consumers, { mapping, nullptr, nullptr, nullptr }, poses, pose_stride_bytes, stream);
}
