// kernels_raw_scalar_tracks.inl -- part of aclhip.hip (one translation unit; included there behind kernels_raw_tracks.inl, not compiled on its own).
// Raw scalar track arrays: sample_raw_scalar_tracks_kernel (aclhip_sample_raw_scalar_tracks_batch), sample_raw_scalar_track_kernel
// (aclhip_sample_raw_scalar_track_batch) -- acl::track_array's sample_tracks and sample_track (compression/impl/track_array.impl.h:209-438)
// for float1f .. vector4f of UNCOMPRESSED curve sets, batched -- and measure_scalar_error_kernel (aclhip_measure_scalar_error_batch):
// calculate_scalar_track_error (compression/impl/track_error.impl.h:53-103, :198-213) over two value buffers. include/aclhip.h states
// the definitions.

	// A raw scalar track array's record in the context's table (a table of its own: no handle of one kind names an array of the other)
	// and its device image: the caller's [num_samples][num_tracks][C] floats as they were handed over, sample major and tight -- one key
	// frame of the whole list is one contiguous run of num_tracks * C floats, the layout of the row the launch writes. A cleared record
	// (samples == null) is an unknown or retired handle; record 0 is never handed out.
	struct device_raw_scalar_tracks
	{
		const float* samples;				// [num_samples][num_tracks * num_components]
		uint32_t num_tracks;
		uint32_t num_samples;
		float sample_rate;
		float duration;						// calculate_finite_duration(num_samples + (wrap ? 1 : 0), sample_rate), made on the host
		uint32_t looping_policy;			// k_loop_clamp or k_loop_wrap | acl::track_type8 << 8 (float4f and vector4f both hold 4 floats: the compressor's header names the type)
		uint32_t num_components;			// C: 1 to 4
	};
	static_assert(sizeof(device_raw_scalar_tracks) == 32, "load_entry: two dwordx4 loads");

	// the record with every field in scalar registers of its own (load_skeleton_fields, kernels_skeleton.inl, says why)
	__device__ __forceinline__ device_raw_scalar_tracks load_raw_scalar_tracks_fields(const device_raw_scalar_tracks* table, uint32_t index)
	{
		device_raw_scalar_tracks raw = load_entry(table, index);
		asm volatile("" : "+s"(raw.samples), "+s"(raw.num_tracks), "+s"(raw.num_samples), "+s"(raw.sample_rate), "+s"(raw.duration), "+s"(raw.looping_policy), "+s"(raw.num_components));
		return raw;
	}

	__device__ __forceinline__ uint32_t raw_scalar_looping_policy_of(const device_raw_scalar_tracks& raw) { return raw.looping_policy & 0xFFu; }
	__device__ __forceinline__ uint32_t raw_scalar_track_type_of(const device_raw_scalar_tracks& raw) { return raw.looping_policy >> 8; }

	// the argument of both sampling kernels
	struct raw_scalar_sample_launch
	{
		const device_raw_scalar_tracks* arrays;		// the context's raw scalar track table
		uint32_t num_arrays;						// its capacity
		uint32_t num_instances;
		const uint32_t* raws;						// [num_instances] handles
		const float* sample_times;					// [num_instances]
		const uint32_t* track_indices;				// [num_instances]; the single-track kernel only
		const uint32_t* rows;						// [num_instances] or null: row i
		const uint8_t* instance_rounding_policies;	// [num_instances] or null: rounding_policy
		const uint8_t* track_rounding_policies;		// [num_track_rounding_policies] or null
		uint32_t num_track_rounding_policies;
		uint32_t rounding_policy;
		uint8_t* values;							// row r at values + r * stride_bytes
		uint64_t stride_bytes;
		uint32_t waves_per_instance;				// the waves that share an instance's elements, 64 lanes at a time in turn (the whole-list kernel only)
		uint32_t dword_only;						// measurement knob (launch_raw_scalar_sample): never the 16 byte path
		unsigned long long* rejected_count;
	};

	constexpr uint32_t k_raw_scalar_waves_per_block = 4;
	constexpr uint32_t k_raw_scalar_elements_per_lane = 16;		// the floats of a row one lane takes in turn, at most: a wave per 4 KiB of row

	// the track an element of a row belongs to: C is wave uniform, and only 3 needs a division (by a constant)
	__device__ __forceinline__ uint32_t raw_scalar_track_of(uint32_t element, uint32_t num_components)
	{
		return num_components == 3u ? element / 3u : element >> (num_components >> 1);		// 1, 2, 4: a shift by 0, 1, 2
	}

	// One wave64 per (instance, share of its row); no LDS, no barrier: sample_raw_tracks_kernel's shape.
	//   scalar unit   the instance's handle, sample time, row and policy, the array's record, the refusal (in front of any load of a key
	//                 frame) and the seek: find_key_frames with ROUND_NONE gives the two key frames and the UNROUNDED alpha
	//   lanes         element e of a row is component e % C of track e / C. Row base, stride and T * C are only 4 byte aligned in general:
	//                 dword   a lane owns one FLOAT of the row: one dword load from each key frame at the same element index, the track's
	//                         rounding of the alpha, the interpolation, one dword streaming store; a wave's accesses are 256 byte
	//                         contiguous pieces whatever the alignment. Serves every case.
	//                 wide    a lane owns four consecutive floats: 16 byte loads and one 16 byte store. Taken by a wave only when the
	//                         addresses of its row and of BOTH key frames are 16 byte aligned -- wave uniform, decided on the scalar unit
	//                         from the addresses themselves --, over the row's whole quads; the last T * C % 4 floats go the dword way.
	//                         With C == 3 (and under PER_TRACK with C < 4) a quad straddles tracks: each of its floats has its own alpha.
	__global__ __launch_bounds__(k_raw_scalar_waves_per_block * k_wave_size) void sample_raw_scalar_tracks_kernel(raw_scalar_sample_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t wave = blockIdx.x * k_raw_scalar_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		const uint32_t instance = wave / launch.waves_per_instance;
		const uint32_t share = wave - instance * launch.waves_per_instance;
		if (instance >= launch.num_instances)
			return;

		const uint32_t handle = as_constant(launch.raws)[instance];
		const float sample_time = as_constant(launch.sample_times)[instance];
		const uint32_t row = launch.rows != nullptr ? as_constant(launch.rows)[instance] : instance;
		const uint32_t policy = uniform_instance_byte(launch.instance_rounding_policies, instance, launch.arrays, launch.rounding_policy);
		const device_raw_scalar_tracks raw = load_raw_scalar_tracks_fields(launch.arrays, handle < launch.num_arrays ? handle : 0);
		const uint32_t num_tracks = raw.num_tracks;
		const uint32_t num_components = raw.num_components;
		const uint32_t num_elements = num_tracks * num_components;		// < 2^18

		// refused, wave uniform and in front of any load of a key frame; counted once per instance
		const bool refused = handle >= launch.num_arrays || raw.samples == nullptr || uint64_t(num_elements) * 4u > launch.stride_bytes
			|| (policy == k_round_per_track && num_tracks > launch.num_track_rounding_policies);
		if (refused)
		{
			if (share == 0 && lane == 0)
				atomicAdd(launch.rejected_count, 1ull);
			return;
		}

		// what is served reads inside its two key frames (both < num_samples) and writes inside the first 4 * C * num_tracks bytes of its row
		uint32_t key_frame0, key_frame1;
		float alpha;
		find_key_frames(0, raw.num_samples, raw.sample_rate, raw.duration, raw.duration, sample_time, k_round_none, raw_scalar_looping_policy_of(raw) == k_loop_wrap ? k_loop_wrap : k_loop_clamp,
			key_frame0, key_frame1, alpha);
		key_frame0 = min(key_frame0, raw.num_samples - 1u);		// (sample_raw_tracks_kernel says when)

		const ACLHIP_CONSTANT float* frame0 = as_constant(raw.samples) + size_t(key_frame0) * num_elements;
		const ACLHIP_CONSTANT float* frame1 = as_constant(raw.samples) + size_t(key_frame1) * num_elements;
		float* out = reinterpret_cast<float*>(launch.values + uint64_t(row) * launch.stride_bytes);
		const bool per_track = policy == k_round_per_track;

		uint32_t first_dword_element = 0;
		const bool wide = ((reinterpret_cast<uintptr_t>(frame0) | reinterpret_cast<uintptr_t>(frame1) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0 && launch.dword_only == 0;
		if (wide)
		{
			const uint32_t num_quads = num_elements / 4u;
			const ACLHIP_CONSTANT f32x4* quads0 = reinterpret_cast<const ACLHIP_CONSTANT f32x4*>(frame0);
			const ACLHIP_CONSTANT f32x4* quads1 = reinterpret_cast<const ACLHIP_CONSTANT f32x4*>(frame1);
			const float uniform_alpha = apply_rounding_policy(alpha, policy);		// (PER_TRACK rounds nothing here)
			for (uint32_t quad = share * k_wave_size + lane; quad < num_quads; quad += launch.waves_per_instance * k_wave_size)
			{
				const f32x4 v0 = quads0[quad], v1 = quads1[quad];
				float a[4] = { uniform_alpha, uniform_alpha, uniform_alpha, uniform_alpha };
				if (per_track)
				{
					#pragma unroll
					for (uint32_t k = 0; k < 4; ++k)
						a[k] = apply_rounding_policy(alpha, uint32_t(as_constant(launch.track_rounding_policies)[raw_scalar_track_of(quad * 4u + k, num_components)]));
				}
				store_streaming(reinterpret_cast<f32x4*>(out) + quad,
					f32x4{ lerp_stable(v0.x, v1.x, a[0]), lerp_stable(v0.y, v1.y, a[1]), lerp_stable(v0.z, v1.z, a[2]), lerp_stable(v0.w, v1.w, a[3]) });
			}
			first_dword_element = num_quads * 4u;		// at most three floats remain
		}

		for (uint32_t element = first_dword_element + share * k_wave_size + lane; element < num_elements; element += launch.waves_per_instance * k_wave_size)
		{
			const float v0 = frame0[element], v1 = frame1[element];
			const uint32_t track = raw_scalar_track_of(element, num_components);
			const float track_alpha = apply_rounding_policy(alpha, per_track ? uint32_t(as_constant(launch.track_rounding_policies)[track]) : policy);
			const float result[1] = { lerp_stable(v0, v1, track_alpha) };
			store_streaming_floats(out + element, result);
		}
	}

	// track_array::sample_track: one THREAD per request (every lane has its own array, time and track; a wave works on 64 requests
	// together, like decompress_scalar_track_kernel): C floats at values + row * stride. The alpha is the unrounded one of the seek,
	// rounded with the request's policy -- the reference hands that policy to the key frame search, which rounds with the same
	// apply_rounding_policy: the bits are the whole-list kernel's for that track.
	__global__ __launch_bounds__(k_raw_scalar_waves_per_block * k_wave_size) void sample_raw_scalar_track_kernel(raw_scalar_sample_launch launch)
	{
		const uint32_t instance = blockIdx.x * (k_raw_scalar_waves_per_block * k_wave_size) + threadIdx.x;
		if (instance >= launch.num_instances)
			return;

		const uint32_t handle = launch.raws[instance];
		const uint32_t track = launch.track_indices[instance];
		const uint32_t policy = launch.instance_rounding_policies != nullptr ? uint32_t(launch.instance_rounding_policies[instance]) : launch.rounding_policy;
		const device_raw_scalar_tracks raw = launch.arrays[handle < launch.num_arrays ? handle : 0];
		const uint32_t num_components = raw.num_components;

		// refused in front of any load of a key frame, counted per request
		const bool refused = handle >= launch.num_arrays || raw.samples == nullptr || track >= raw.num_tracks || uint64_t(num_components) * 4u > launch.stride_bytes
			|| (policy == k_round_per_track && track >= launch.num_track_rounding_policies);
		if (refused)
		{
			atomicAdd(launch.rejected_count, 1ull);
			return;
		}

		uint32_t key_frame0, key_frame1;
		float alpha;
		find_key_frames(0, raw.num_samples, raw.sample_rate, raw.duration, raw.duration, launch.sample_times[instance], k_round_none,
			raw_scalar_looping_policy_of(raw) == k_loop_wrap ? k_loop_wrap : k_loop_clamp, key_frame0, key_frame1, alpha);
		key_frame0 = min(key_frame0, raw.num_samples - 1u);
		alpha = apply_rounding_policy(alpha, policy == k_round_per_track ? uint32_t(launch.track_rounding_policies[track]) : policy);

		const uint32_t num_elements = raw.num_tracks * num_components;
		const float* v0 = raw.samples + size_t(key_frame0) * num_elements + track * num_components;
		const float* v1 = raw.samples + size_t(key_frame1) * num_elements + track * num_components;
		const uint32_t row = launch.rows != nullptr ? launch.rows[instance] : instance;
		float* out = reinterpret_cast<float*>(launch.values + uint64_t(row) * launch.stride_bytes);
		// (component by component: a track of a tight list is only 4 byte aligned, and so is the row)
		for (uint32_t component = 0; component < num_components; ++component)
		{
			const float result[1] = { lerp_stable(v0[component], v1[component], alpha) };
			store_streaming_floats(out + component, result);
		}
	}

	// ---- how far two value buffers are apart (aclhip_measure_scalar_error_batch) ----------------------------------------------------------
	struct scalar_error_launch
	{
		const uint8_t* raw_values;
		uint64_t raw_stride_bytes;
		const uint8_t* lossy_values;
		uint64_t lossy_stride_bytes;
		uint8_t* track_errors;				// or null
		uint64_t track_error_stride_bytes;
		pose_error_record* errors;			// [num_instances]: aclhip_track_error has aclhip_pose_error's layout
		uint32_t num_instances;
		uint32_t num_tracks;
		uint32_t num_components;
	};

	constexpr uint32_t k_scalar_error_waves_per_block = 4;

	// One wave64 per instance: a lane takes tracks lane, lane + 64, ... in ascending order and keeps the first of its greatest errors (a
	// strict >: a NaN never wins, ties stay with the lower track), then wave_reduce_worst, whose tie rule prefers the lower track too.
	// Every lane's record starts at { -1, k_no_bone }: no error in the reduction is a NaN.
	__global__ __launch_bounds__(k_scalar_error_waves_per_block * k_wave_size) void measure_scalar_error_kernel(scalar_error_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t instance = blockIdx.x * k_scalar_error_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		if (instance >= launch.num_instances)
			return;

		const float* raw_row = reinterpret_cast<const float*>(launch.raw_values + uint64_t(instance) * launch.raw_stride_bytes);
		const float* lossy_row = reinterpret_cast<const float*>(launch.lossy_values + uint64_t(instance) * launch.lossy_stride_bytes);
		float* track_errors = launch.track_errors != nullptr ? reinterpret_cast<float*>(launch.track_errors + uint64_t(instance) * launch.track_error_stride_bytes) : nullptr;
		const uint32_t num_components = launch.num_components;

		float worst_error = -1.0f;
		uint32_t worst_track = k_no_bone, unused_payload = 0;
		for (uint32_t track = lane; track < launch.num_tracks; track += k_wave_size)
		{
			const size_t first = size_t(track) * num_components;
			// max(a, b) = a > b ? a : b in ascending component order would drop a NaN; a NaN component makes the track's error a NaN
			float error = fabsf(raw_row[first] - lossy_row[first]);
			bool is_nan = error != error;
			for (uint32_t component = 1; component < num_components; ++component)
			{
				const float component_error = fabsf(raw_row[first + component] - lossy_row[first + component]);
				is_nan = is_nan || component_error != component_error;
				error = error > component_error ? error : component_error;
			}
			error = is_nan ? __uint_as_float(0x7FC00000u) : error;
			if (track_errors != nullptr)
				track_errors[track] = error;
			if (error > worst_error)
			{
				worst_error = error;
				worst_track = track;
			}
		}
		wave_reduce_worst(worst_error, worst_track, unused_payload);
		if (lane == 0)
			launch.errors[instance] = pose_error_record{ worst_error, worst_track };
	}
