// host_bone_object.inl -- part of aclhip.hip (one translation unit; included there, in this order, not compiled on its own).
// Host side of the single bone requests in object space: the chain planner and the two launches (kernels_bone_object.inl).

extern "C" aclhip_status aclhip_plan_bone_chain(const uint32_t* parent_indices, uint32_t num_tracks, uint32_t bone, uint32_t* out_chain, uint32_t chain_capacity, uint32_t* out_length)
{
	if (parent_indices == nullptr || out_length == nullptr || bone >= num_tracks)
		return ACLHIP_ERROR_INVALID_ARGUMENT;
	return guarded(nullptr, [&]() -> aclhip_status
	{
		// the rules of aclhip_set_clip_hierarchy, for the whole hierarchy: a chain through a misplaced transform elsewhere is refused too
		hierarchy_tree tree;
		uint32_t misplaced = 0;
		if (!build_hierarchy_tree(parent_indices, num_tracks, tree, misplaced))
			return ACLHIP_ERROR_INVALID_ARGUMENT;
		uint32_t length = 1;
		for (uint32_t transform = bone; !tree.is_root[transform]; transform = parent_indices[transform])
			length++;
		*out_length = length;
		if (out_chain == nullptr)
			return ACLHIP_OK;
		if (chain_capacity < length)
			return ACLHIP_ERROR_INVALID_ARGUMENT;
		uint32_t transform = bone;
		for (uint32_t position = length; position-- > 0;)
		{
			out_chain[position] = transform;
			if (position != 0)		// (a root's parent index is not read)
				transform = parent_indices[transform];
		}
		return ACLHIP_OK;
	});
}

namespace
{
	// mapping == nullptr: the unmapped form, the chain over the clip's own hierarchy
	aclhip_status launch_bone_requests(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* bones, uint32_t num_requests,
		const aclhip_decompress_params* params, const aclhip_pose_mapping* mapping, bool mapped, void* transforms, void* stream)
	{
		aclhip_status status = check_batch_arguments(context, clips, sample_times, num_requests, transforms, 48);
		if (status != ACLHIP_OK)
			return status;
		if (mapped)
		{
			if (mapping == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null pose mapping");
			if (mapping->skeleton == 0 && mapping->instance_skeletons == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a pose mapping names a skeleton or a list of skeletons");
			if (mapping->map == 0 && mapping->instance_maps == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a pose mapping names a map or a list of maps");
			if (mapping->blend_maps != nullptr || mapping->base_maps != nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "single bone requests take no blend and no base: blend_maps and base_maps are NULL");
		}
		if (num_requests == 0)
			return ACLHIP_OK;
		if (bones == nullptr)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, mapped ? "null bone slot list" : "null track index list");

		decode_params device_params;
		status = resolve_params(context, params, device_params);
		if (status != ACLHIP_OK)
			return status;
		// every local transform of the chain whole, as the pose consumers' images hold it
		if (device_params.standard_defaults == 0 || device_params.per_track_rounding != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "object space requests take the track_writer's default sub-track modes, no per track rounding, normalization != always");

		std::shared_lock<std::shared_mutex> lock(context->mutex);		// see launch_tracks
		skeleton_launch device_mapping = {};
		if (mapped)
		{
			if (context->skeletons.d_records == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no skeleton was ever registered with this context");
			if (context->track_maps.d_records == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "no track map was ever registered with this context");
			device_mapping.skeletons = context->skeletons.d_records;
			device_mapping.num_skeletons = ACLHIP_MAX_SKELETONS;
			device_mapping.maps = context->track_maps.d_records;
			device_mapping.num_maps = ACLHIP_MAX_TRACK_MAPS;
			device_mapping.skeleton = mapping->skeleton;
			device_mapping.map = mapping->map;
			device_mapping.instance_skeletons = mapping->instance_skeletons;
			device_mapping.instance_maps = mapping->instance_maps;
		}
		device_guard guard(context->device);
		note_launch_stream(context, static_cast<hipStream_t>(stream));

		// rtm::qvv_mul's matrix route only while something registered can hand out a negative scale (launch_consumers' rule)
		const bool mirrored = context->num_negative_scale_clips != 0 || (mapped && context->num_negative_scale_skeletons != 0);
		typedef void (*bone_kernel)(const device_clip*, uint32_t, const uint32_t*, const float*, const uint32_t*, uint32_t, decode_params, float4*, unsigned long long*, skeleton_launch);
		static const bone_kernel kernels[2][2] =
		{
			{ decompress_bone_object_kernel<false, false>, decompress_bone_object_kernel<false, true> },
			{ decompress_bone_object_kernel<true, false>, decompress_bone_object_kernel<true, true> },
		};
		const uint32_t num_blocks = (num_requests + k_block_size - 1) / k_block_size;
		hipLaunchKernelGGL(kernels[mapped ? 1 : 0][mirrored ? 1 : 0], dim3(num_blocks), dim3(k_block_size), 0, static_cast<hipStream_t>(stream),
			context->d_clips, context->d_clips_capacity, clips, sample_times, bones, num_requests, device_params,
			static_cast<float4*>(transforms), context->d_rejected, device_mapping);
		ACLHIP_CHECK_HIP(context, hipGetLastError());
		return ACLHIP_OK;
	}
}

extern "C" aclhip_status aclhip_decompress_track_object_batch(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* track_indices,
	uint32_t num_requests, const aclhip_decompress_params* params, void* transforms, void* stream)
{
	return launch_bone_requests(context, clips, sample_times, track_indices, num_requests, params, nullptr, false, transforms, stream);
}

extern "C" aclhip_status aclhip_decompress_bone_object_batch_mapped(aclhip_context* context, const aclhip_clip* clips, const float* sample_times, const uint32_t* bone_slots,
	uint32_t num_requests, const aclhip_decompress_params* params, const aclhip_pose_mapping* mapping, void* transforms, void* stream)
{
	return launch_bone_requests(context, clips, sample_times, bone_slots, num_requests, params, mapping, true, transforms, stream);
}
