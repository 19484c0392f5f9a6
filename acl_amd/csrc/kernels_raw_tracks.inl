// kernels_raw_tracks.inl -- part of aclhip.hip (one translation unit; included there behind kernels_pose_buffers.inl, not compiled on its own).
// Raw track arrays: sample_raw_tracks_kernel (aclhip_sample_raw_tracks_batch; include/aclhip.h states the definition) --
// acl::track_array_qvvf::sample_tracks (compression/impl/track_array.impl.h:209-343) of UNCOMPRESSED clips, batched.

	// A raw track array's record in the context's table (which never moves, like the skin table) and its device image: the caller's
	// [num_samples][num_tracks] QVV48 records as they were handed over, sample major -- one key frame of the whole pose is one contiguous
	// run of 3 * num_tracks quads, so a wave's loads of a key frame are as contiguous as its stores of the row. A cleared record
	// (samples == null) is an unknown or retired handle; record 0 is never handed out.
	struct device_raw_tracks
	{
		const f32x4* samples;				// [num_samples][3 * num_tracks] rotation | translation | scale quads, lane 3 as the caller left it
		uint32_t num_tracks;
		uint32_t num_samples;
		float sample_rate;
		float duration;						// calculate_finite_duration(num_samples + (wrap ? 1 : 0), sample_rate), made on the host
		uint32_t looping_policy;			// k_loop_clamp or k_loop_wrap
		uint32_t reserved;
	};
	static_assert(sizeof(device_raw_tracks) == 32, "load_entry: two dwordx4 loads");

	// a raw track array's record with every field in scalar registers of its own (load_skeleton_fields, kernels_skeleton.inl, says why)
	__device__ __forceinline__ device_raw_tracks load_raw_tracks_fields(const device_raw_tracks* table, uint32_t index)
	{
		device_raw_tracks raw = load_entry(table, index);
		asm volatile("" : "+s"(raw.samples), "+s"(raw.num_tracks), "+s"(raw.num_samples), "+s"(raw.sample_rate), "+s"(raw.duration), "+s"(raw.looping_policy));
		return raw;
	}

	// the kernel's argument
	struct raw_sample_launch
	{
		const device_raw_tracks* arrays;			// the context's raw track table
		uint32_t num_arrays;						// its capacity
		uint32_t num_instances;
		const uint32_t* raws;						// [num_instances] handles
		const float* sample_times;					// [num_instances]
		const uint32_t* rows;						// [num_instances] or null: row i
		const uint8_t* instance_rounding_policies;	// [num_instances] or null: rounding_policy
		const uint8_t* track_rounding_policies;		// [num_track_rounding_policies] or null
		uint32_t num_track_rounding_policies;
		uint32_t rounding_policy;
		uint8_t* poses;								// row r at poses + r * pose_stride_bytes: QVV48
		uint64_t pose_stride_bytes;
		uint32_t waves_per_instance;				// the waves that share an instance's quads, 64 at a time in turn
		unsigned long long* rejected_count;
	};

	constexpr uint32_t k_raw_sample_waves_per_block = 4;
	constexpr uint32_t k_raw_sample_quads_per_lane = 8;		// the quads of a row one lane takes in turn, at most (launch_raw_sample, host_raw_tracks.inl, says why)

	// One wave64 per (instance, share of its quads); no LDS, no barrier: the waves of a workgroup have nothing to do with each other.
	//   scalar unit   the instance's handle, sample time, row and policy, the array's record, the refusal (in front of any load of a key
	//                 frame) and the seek: find_key_frames with ROUND_NONE gives the two key frames and the UNROUNDED alpha
	//   lanes         one lane owns one 16 byte quad of the pose row (3 per track, quad % 3 == 0 is a rotation): one 16 byte load from each
	//                 key frame at the same quad index, the track's rounding of the alpha, the interpolation, one 16 byte streaming store.
	//                 Loads and stores of a wave are 1 KiB contiguous pieces.
	// The rotation's arithmetic (a dot product, a square root and a division, correctly rounded: quat_normalize<false> -- nothing is proven
	// about a caller's rotations) sits behind a branch every wave takes with a third of its lanes; the vector lanes wait for it. The waves
	// of an instance take its quads 64 at a time in turn: every load and store of a wave is a contiguous piece of 1 KiB.
	__global__ __launch_bounds__(k_raw_sample_waves_per_block * k_wave_size) void sample_raw_tracks_kernel(raw_sample_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t wave = blockIdx.x * k_raw_sample_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		const uint32_t instance = wave / launch.waves_per_instance;
		const uint32_t share = wave - instance * launch.waves_per_instance;
		if (instance >= launch.num_instances)
			return;

		const uint32_t handle = as_constant(launch.raws)[instance];
		const float sample_time = as_constant(launch.sample_times)[instance];
		const uint32_t row = launch.rows != nullptr ? as_constant(launch.rows)[instance] : instance;
		// (the dword that holds the instance's byte, on the scalar unit: uniform_instance_byte, aclhip_device.h, says why)
		const uint32_t policy = uniform_instance_byte(launch.instance_rounding_policies, instance, launch.arrays, launch.rounding_policy);
		const device_raw_tracks raw = load_raw_tracks_fields(launch.arrays, handle < launch.num_arrays ? handle : 0);
		const uint32_t num_tracks = raw.num_tracks;

		// refused, wave uniform and in front of any load of a key frame; counted once per instance
		const bool refused = handle >= launch.num_arrays || raw.samples == nullptr || uint64_t(num_tracks) * 48u > launch.pose_stride_bytes
			|| (policy == k_round_per_track && num_tracks > launch.num_track_rounding_policies);
		if (refused)
		{
			if (share == 0 && lane == 0)
				atomicAdd(launch.rejected_count, 1ull);
			return;
		}

		// what is served reads inside its two key frames (both < num_samples) and writes inside the first 48 * num_tracks bytes of its row
		uint32_t key_frame0, key_frame1;
		float alpha;
		find_key_frames(0, raw.num_samples, raw.sample_rate, raw.duration, raw.duration, sample_time, k_round_none, raw.looping_policy == k_loop_wrap ? k_loop_wrap : k_loop_clamp,
			key_frame0, key_frame1, alpha);
		// (never taken by a finite time at a rate whose products stay exact enough; a rate so small or an array so long that time * rate
		// rounds past the last sample must still read inside the array)
		key_frame0 = min(key_frame0, raw.num_samples - 1u);

		const uint32_t num_quads = num_tracks * 3u;
		const ACLHIP_CONSTANT f32x4* frame0 = as_constant(raw.samples) + size_t(key_frame0) * num_quads;
		const ACLHIP_CONSTANT f32x4* frame1 = as_constant(raw.samples) + size_t(key_frame1) * num_quads;
		f32x4* out = reinterpret_cast<f32x4*>(launch.poses + uint64_t(row) * launch.pose_stride_bytes);
		const bool per_track = policy == k_round_per_track;

		for (uint32_t quad = share * k_wave_size + lane; quad < num_quads; quad += launch.waves_per_instance * k_wave_size)
		{
			const f32x4 v0 = frame0[quad], v1 = frame1[quad];
			const uint32_t track = quad / 3u;
			const float track_alpha = apply_rounding_policy(alpha, per_track ? uint32_t(as_constant(launch.track_rounding_policies)[track]) : policy);
			f32x4 result;
			if (quad == track * 3u)
			{
				const float4 rotation = quat_normalize<false>(quat_lerp_no_normalization(make_float4(v0.x, v0.y, v0.z, v0.w), make_float4(v1.x, v1.y, v1.z, v1.w), track_alpha));
				result = f32x4{ rotation.x, rotation.y, rotation.z, rotation.w };
			}
			else
				result = f32x4{ lerp_stable(v0.x, v1.x, track_alpha), lerp_stable(v0.y, v1.y, track_alpha), lerp_stable(v0.z, v1.z, track_alpha), 0.0f };
			store_streaming(&out[quad], result);
		}
	}
