// kernels_pose_buffers.inl -- part of aclhip.hip (one translation unit; included there behind kernels_skeleton.inl, not compiled on its own).
// The pose consumers over a CALLER'S pose buffers (aclhip_transform_poses_batch): transform_poses_kernel fills its LDS image from a row
// in HBM instead of from a clip, and everything behind the fill is decompress_poses_consumer_kernel's finish_consumer_poses with the
// skeleton's bone count and walk schedule -- the combine with a base buffer, the walk, the store and the bounds.

	// the kernel's argument: the launch's three buffers, its skeletons and its shape
	struct pose_buffer_launch
	{
		const device_skeleton* skeletons;		// the context's skeleton table
		uint32_t num_skeletons;					// its capacity
		uint32_t skeleton;						// the launch's skeleton, when instance_skeletons is null
		const uint32_t* instance_skeletons;		// [num_instances] or null
		const uint8_t* local_poses;				// row i at local_poses + i * local_pose_stride_bytes
		uint64_t local_pose_stride_bytes;
		const uint8_t* additive_poses;			// kBase == k_consumer_base_buffer: row i at additive_poses + i * additive_pose_stride_bytes
		uint64_t additive_pose_stride_bytes;
		uint8_t* poses;							// null: the boxes alone (bounds instantiations)
		uint64_t pose_stride_bytes;
		uint32_t num_instances;
		uint32_t additive_format;
		uint32_t lds_quads_per_image, lds_bytes_per_instance, packed_block_shape;		// as decompress_poses_consumer_kernel takes them
		unsigned long long* rejected_count;
	};

	// One wave64 per instance, up to 8 instances per workgroup, images as consumer_wave_of lays them out.
	//   kObjectSpace   local_to_object_space with the skeleton's walk schedule
	//   kBase          k_consumer_base_none: the image is the local row L. k_consumer_base_buffer: the image is the ADDITIVE row A, and the
	//                  tail reads L per transform as its base pose buffer -- apply_additive_to_base(format, base = L[b], additive = A[b]),
	//                  the roles aclhip_decompress_poses_batch gives an instance's decoded pose and its base_poses row
	//   bounds_types   nothing, or consumer_bounds_launch (object space): a box per instance next to the rows, or in their place
	// Nothing is known about a caller's poses: rtm::qvv_mul's matrix route is always compiled in (kMirrored, the rule the fused kernels
	// apply when the base is a caller's buffer), and short_exact is 0 -- the walk normalizes with the compiler's correctly rounded sqrt and
	// division, because the short forms give the same bits only for rotations of a squared length in their proven range [1/4, 4].
	// In place (poses == local_poses, equal strides): a wave reads its own instance's rows and no other, and every row of the workgroup is
	// complete in LDS -- behind the tail's barriers -- before the first quad of any of them is stored.
	template<bool kObjectSpace, uint32_t kBase, class... bounds_types>
	__global__ __launch_bounds__(k_consumer_max_instances * k_wave_size) void transform_poses_kernel(pose_buffer_launch launch, bounds_types... bounds_launch)
	{
		static_assert(kBase == k_consumer_base_none || kBase == k_consumer_base_buffer, "the additive pose is a caller's buffer, never a clip");
		static_assert(kObjectSpace || kBase == k_consumer_base_buffer, "local space without an additive buffer: nothing to do");
		constexpr bool with_bounds = sizeof...(bounds_types) != 0;
		// packed_block_shape: log2 of the instances per workgroup (bits 0..7) | words of LDS reserved for the shared walk schedule (bits 8..31)
		const uint32_t log2_instances_per_block = launch.packed_block_shape & 0xFFu;
		__shared__ consumer_walk_slots walk;		// (what the host subtracts from the LDS it may ask for: host_consumers.inl)
		ACLHIP_PHASE_STAMP(0);

		consumer_wave wave = consumer_wave_of(log2_instances_per_block, launch.lds_bytes_per_instance, launch.lds_quads_per_image);
		const uint32_t lane = wave.lane, instance = wave.instance;

		// (wave.num_tracks stays 0 for a wave without work: past the batch, refused instance)
		if (instance < launch.num_instances)
		{
			// the skeleton's record on the scalar unit; record 0 is never handed out and a cleared record is an unknown or retired skeleton
			const uint32_t skeleton_id = launch.instance_skeletons != nullptr ? as_constant(launch.instance_skeletons)[instance] : launch.skeleton;
			const device_skeleton skeleton = load_skeleton_fields(launch.skeletons, skeleton_id < launch.num_skeletons ? skeleton_id : 0);
			const uint32_t num_bones = skeleton.num_bones;
			const uint64_t row_bytes = uint64_t(num_bones) * 48u;

			// refused, wave uniform and in front of any load of a row: an unknown or retired skeleton, object space without a hierarchy, more
			// bones than a row of any buffer in use or the launch's LDS image holds (the image is sized from a stride on the host, and a
			// skeleton may be registered behind a captured launch's back). What is served reads and writes inside its own rows.
			const bool refused = skeleton_id >= launch.num_skeletons || skeleton.reference_pose == nullptr || (kObjectSpace && skeleton.hierarchy == nullptr)
				|| row_bytes > launch.local_pose_stride_bytes || (launch.poses != nullptr && row_bytes > launch.pose_stride_bytes)
				|| (kBase == k_consumer_base_buffer && row_bytes > launch.additive_pose_stride_bytes) || num_bones * 3u > launch.lds_quads_per_image;
			if (refused)
			{
				if (lane == 0)
					atomicAdd(launch.rejected_count, 1ull);
			}
			else if (num_bones != 0)
			{
				wave.num_tracks = num_bones;
				// the walk schedule first: its words travel global -> LDS while the row does
				if (kObjectSpace)
					request_walk_schedule(skeleton.hierarchy, log2_instances_per_block, launch.packed_block_shape >> 8, wave.shared_schedule, wave.slot, lane, walk);
				// the row straight into the image by DMA, lanes <-> consecutive quads (the LDS side of a piece is wave uniform + lane * 16);
				// the tail's first barrier waits for it (vmcnt) in front of the first LDS read
				const uint8_t* row = kBase == k_consumer_base_buffer ? launch.additive_poses + uint64_t(instance) * launch.additive_pose_stride_bytes
					: launch.local_poses + uint64_t(instance) * launch.local_pose_stride_bytes;
				const f32x4* source = reinterpret_cast<const f32x4*>(row);
				const uint32_t num_quads = num_bones * 3u;
				for (uint32_t base = 0; base < num_quads; base += k_wave_size)
				{
					if (base + lane < num_quads)
						__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(source + base + lane),
							(__attribute__((address_space(3))) void*)(wave.image + base), 16, 0, 0);
				}
			}
			else if constexpr (with_bounds)
				wave.empty_pose = true;		// (a served instance whose pose has no transform)
		}

		// the image of every instance is complete
		wave.short_exact = 0;
		const consumer_bounds_launch bounds = bounds_launch_of(bounds_launch...);
		finish_consumer_poses<kObjectSpace, kBase, false, true, false, with_bounds>(
			consumer_tail_args{ launch.poses, launch.pose_stride_bytes, launch.lds_bytes_per_instance, log2_instances_per_block, launch.rejected_count, launch.local_poses, launch.local_pose_stride_bytes,
				launch.additive_format, bounds.bounds, bounds.bone_flags },
			wave, walk);
	}
