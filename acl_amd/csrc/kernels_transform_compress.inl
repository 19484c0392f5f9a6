// kernels_transform_compress.inl -- part of aclhip.hip (one translation unit; included there behind kernels_scalar_compress.inl, not compiled on its own).
// aclhip_compress_raw_tracks_batch: acl::compress_track_list for a track_array_qvvf with the reference's RAW compression settings
// (quatf_full / vector3f_full / vector3f_full; compression/impl/compress.transform.impl.h:138-530 and the files it calls) over a batch of
// raw track arrays, in four stream ordered launches -- the data dependences set the cuts:
//   transform_compress_analyze_kernel   per (instance, track): the finite test, the normalized test, constant and default per sub-track:
//                                       one flag byte per track, no atomics
//   transform_compress_layout_kernel    per instance: the statuses, the counts, the size, the refusal against the stride, the headers, the
//                                       packed sub-track types, the constant samples, the metadata, the tail; the compact per-type lists of
//                                       animated tracks for the stream
//   transform_compress_stream_kernel    per output dword of the animated stream: one 4 byte load, a byte swap, one coalesced store
//   compress_hash_kernel                (kernels_scalar_compress.inl: both compressors') FNV-1a 32 over [8, size)
// include/aclhip.h states the definition. No float arithmetic touches a stored value: the only arithmetic is the normalized test, one IEEE
// operation at a time in the order of the reference's dot product.
// The layout and the stream kernel are templates: their <true> instantiations are aclhip_compress_tracks_batch's (kernels_tracks_compress.inl)
// for quatf_drop_w_full -- three words per rotation, normalized and of positive w --, their <false> ones this call's, unchanged.

	// What the launches hand to each other, in the caller's workspace: the 64 byte compress_instance per instance (the hash kernel reads
	// status and size out of it; num_animated / num_animated_translations / num_animated_scales hold the animated rotation / translation /
	// scale counts, num_bits_per_frame the bits of one animated pose), one flag byte per (instance, track) and three lists of 16 bit track
	// indices per instance. Every byte that is read was written by an earlier launch of the same call.
	constexpr uint32_t k_transform_flag_not_finite = 0x40;			// bits 0-1 / 2-3 / 4-5: the rotation / translation / scale sub-track type
	constexpr uint32_t k_transform_flag_not_normalized = 0x80;
	constexpr uint32_t k_compress_status_not_normalized = 4;		// (behind k_compress_status_not_finite and k_compress_status_refused)
	constexpr uint32_t k_compress_include_parents = 2;				// ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES
	constexpr uint32_t k_compress_include_descriptions = 4;			// ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS
	constexpr uint32_t k_transform_blob_headers = 100;				// raw_buffer_header, tracks_header, transform_tracks_header, one segment_header

	struct transform_compress_launch
	{
		const device_raw_tracks* arrays;			// the context's raw track table
		uint32_t num_arrays;
		uint32_t num_instances;
		const uint32_t* raws;						// [num_instances] handles
		const f32x4* default_pose;					// [table_tracks][3] QVV48 or null: the identity
		const uint32_t* parent_indices;				// [table_tracks] or null: every track a root
		const float* track_precisions;				// [table_tracks] or null: precision
		const float* track_shell_distances;			// [table_tracks] or null: shell_distance
		uint32_t table_tracks;						// entries of every table above; 0xFFFFFFFF when there is none
		uint32_t flags;								// k_compress_include_*: descriptions imply parents
		float precision;
		float shell_distance;
		uint32_t max_tracks;
		uint32_t waves_per_instance;				// the stream kernel's
		compress_instance* instances;				// [num_instances]
		uint8_t* track_flags;						// [num_instances][max_tracks]
		uint16_t* animated;							// [num_instances][3][max_tracks]: the animated tracks of a type, ascending
		uint8_t* blobs;
		uint64_t blob_stride_bytes;
		uint2* results;								// [num_instances] aclhip_compress_result
		unsigned long long* rejected_count;
		// aclhip_compress_tracks_batch alone (kernels_tracks_compress.inl), behind everything the raw call reads
		float2* shells;								// [num_instances][max_tracks] { local shell distance, precision } of the rigid shell
		float2* shell_metadata;						// the caller's copy of them, or null
		// the _additive entry points alone (kernels_tracks_compress.inl: compress_additive_base), behind everything the others read
		const uint32_t* base_raws;					// [num_instances] handles of the instances' bases, or null: additive_format is 0
		uint32_t additive_format;					// an aclhip_additive_format; 0 (none) in every other call
	};

	// the default-scale bit of the header's word 7: default scale 0 under additive1, 1 otherwise (compress.transform.impl.h:422-423)
	__device__ __forceinline__ uint32_t transform_compress_default_scale_bit(const transform_compress_launch& launch) { return launch.additive_format == 3 ? 0u : 2u; }

	// wave uniform, decided from the handle, the record and the launch alone: the analysis and the layout come to the same answer
	__device__ __forceinline__ bool transform_compress_refused(const transform_compress_launch& launch, uint32_t handle, const device_raw_tracks& raw)
	{
		return handle >= launch.num_arrays || raw.samples == nullptr || raw.num_tracks > launch.max_tracks || raw.num_tracks > launch.table_tracks;
	}

	// a track's settings: its table's entry, or the desc's value; its parent as given, and as an output index (the identity map here: a
	// parent that is no track of the array is no parent)
	__device__ __forceinline__ float compress_track_precision(const transform_compress_launch& launch, uint32_t track) { return launch.track_precisions != nullptr ? launch.track_precisions[track] : launch.precision; }
	__device__ __forceinline__ float compress_track_shell_distance(const transform_compress_launch& launch, uint32_t track) { return launch.track_shell_distances != nullptr ? launch.track_shell_distances[track] : launch.shell_distance; }
	__device__ __forceinline__ uint32_t compress_track_parent(const transform_compress_launch& launch, uint32_t track) { return launch.parent_indices != nullptr ? launch.parent_indices[track] : ACLHIP_NO_PARENT; }
	__device__ __forceinline__ uint32_t compress_track_parent(const transform_compress_launch& launch, uint32_t track, uint32_t num_tracks)
	{
		const uint32_t parent = compress_track_parent(launch, track);
		return parent < num_tracks ? parent : ACLHIP_NO_PARENT;
	}

	__device__ __forceinline__ bool transform_compress_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

	// 0 default, 1 constant, 2 animated
	__device__ __forceinline__ uint32_t transform_compress_type(bool constant, bool is_default) { return constant ? (is_default ? k_sub_track_default : k_sub_track_constant) : k_sub_track_animated; }

	// quatf_drop_w_full (aclhip_compress_tracks_batch; include/aclhip.h states the definition): every rotation normalized with the
	// correctly rounded 1 / sqrt over vector_dot's lane order, and, where it is stored or compared, of positive w (convert_rotation.transform.h:93-96:
	// the sign bit of w xored into all four lanes, a w of -0 included)
	__device__ __forceinline__ float4 tracks_compress_normalize(f32x4 q)
	{
		const float inv_length = 1.0f / sqrtf((q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w));
		return make_float4(q.x * inv_length, q.y * inv_length, q.z * inv_length, q.w * inv_length);
	}

	__device__ __forceinline__ float4 tracks_compress_positive_w(float4 q)
	{
		const uint32_t sign = __float_as_uint(q.w) & 0x80000000u;
		return make_float4(__uint_as_float(__float_as_uint(q.x) ^ sign), __uint_as_float(__float_as_uint(q.y) ^ sign), __uint_as_float(__float_as_uint(q.z) ^ sign),
			__uint_as_float(__float_as_uint(q.w) ^ sign));
	}

	// ---- per (instance, track): the checks and the three sub-track types ----------------------------------------------------------------------
	// One wave64 per track, samples across the lanes: a lane takes the three quads of its sample's record (a track's records lie 48 T bytes
	// apart: the four waves of a block take neighbouring tracks and share the lines) and compares them with sample 0's, which every lane
	// loads from the same address. blockIdx.y walks the instances. The fourth lanes of translations and scales are loaded and never used.
	//   finite       the four rotation lanes, translation and scale xyz
	//   normalized   rtm::quat_is_normalized: fabs(((x * x + z * z) + (y * y + w * w)) - 1) < 0.00001F -- vector_dot's lane order
	//   constant     every sample == sample 0 in every used lane (-0 == +0); default: constant and sample 0 == the default value
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void transform_compress_analyze_kernel(transform_compress_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t track = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		for (uint32_t instance = blockIdx.y; instance < launch.num_instances; instance += gridDim.y)
		{
			const uint32_t handle = as_constant(launch.raws)[instance];
			const device_raw_tracks raw = load_raw_tracks_fields(launch.arrays, handle < launch.num_arrays ? handle : 0);
			if (transform_compress_refused(launch, handle, raw) || track >= raw.num_tracks)
				continue;

			const size_t pose_quads = size_t(raw.num_tracks) * 3u;
			const f32x4* base = raw.samples + size_t(track) * 3u;
			const f32x4 rotation0 = base[0], translation0 = base[1], scale0 = base[2];
			bool finite = true, normalized = true, same_rotation = true, same_translation = true, same_scale = true;
			for (uint32_t sample = lane; sample < raw.num_samples; sample += k_wave_size)
			{
				const f32x4* record = base + sample * pose_quads;
				const f32x4 q = record[0], t = record[1], s = record[2];
				finite = finite && transform_compress_finite(q.x) && transform_compress_finite(q.y) && transform_compress_finite(q.z) && transform_compress_finite(q.w)
					&& transform_compress_finite(t.x) && transform_compress_finite(t.y) && transform_compress_finite(t.z)
					&& transform_compress_finite(s.x) && transform_compress_finite(s.y) && transform_compress_finite(s.z);
				const float length_squared = (q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w);
				normalized = normalized && fabsf(length_squared - 1.0f) < 0.00001f;
				same_rotation = same_rotation && q.x == rotation0.x && q.y == rotation0.y && q.z == rotation0.z && q.w == rotation0.w;
				same_translation = same_translation && t.x == translation0.x && t.y == translation0.y && t.z == translation0.z;
				same_scale = same_scale && s.x == scale0.x && s.y == scale0.y && s.z == scale0.z;
			}

			f32x4 default_rotation = { 0.0f, 0.0f, 0.0f, 1.0f }, default_translation = { 0.0f, 0.0f, 0.0f, 0.0f }, default_scale = { 1.0f, 1.0f, 1.0f, 0.0f };
			if (launch.default_pose != nullptr)
			{
				default_rotation = launch.default_pose[size_t(track) * 3u];
				default_translation = launch.default_pose[size_t(track) * 3u + 1u];
				default_scale = launch.default_pose[size_t(track) * 3u + 2u];
			}
			const bool default_rotation_at_0 = rotation0.x == default_rotation.x && rotation0.y == default_rotation.y && rotation0.z == default_rotation.z && rotation0.w == default_rotation.w;
			const bool default_translation_at_0 = translation0.x == default_translation.x && translation0.y == default_translation.y && translation0.z == default_translation.z;
			const bool default_scale_at_0 = scale0.x == default_scale.x && scale0.y == default_scale.y && scale0.z == default_scale.z;

			uint32_t flags = transform_compress_type(__ballot(!same_rotation) == 0, default_rotation_at_0)
				| (transform_compress_type(__ballot(!same_translation) == 0, default_translation_at_0) << 2)
				| (transform_compress_type(__ballot(!same_scale) == 0, default_scale_at_0) << 4);
			flags |= __ballot(!finite) != 0 ? k_transform_flag_not_finite : 0u;
			flags |= __ballot(!normalized) != 0 ? k_transform_flag_not_normalized : 0u;
			if (lane == 0)
				launch.track_flags[size_t(instance) * launch.max_tracks + track] = uint8_t(flags);
		}
	}

	// the lanes below this one whose bit is set in a ballot
	__device__ __forceinline__ uint32_t transform_compress_rank(uint64_t mask)
	{
		return __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0u));
	}

	// a lane's 2 bit type into its place of the packed word of its 16 lanes (the first track in the top bits); every lane of the 16 gets the word
	__device__ __forceinline__ uint32_t transform_compress_pack_types(uint32_t type, uint32_t lane)
	{
		uint32_t word = type << ((15u - (lane & 15u)) * 2u);
		#pragma unroll
		for (int offset = 1; offset < 16; offset <<= 1)
			word |= uint32_t(__shfl_xor(int(word), offset));
		return word;
	}

	// What an instance that ends with a status leaves for the caller: the result word, no size, and the refusal counted. One lane's.
	__device__ __forceinline__ void compress_write_refusal(const transform_compress_launch& launch, uint32_t instance, uint32_t status)
	{
		// NOT_FINITE wins over NOT_NORMALIZED: the reference tests what it would store
		const uint32_t result = (status & k_compress_status_refused) != 0 ? ACLHIP_COMPRESS_REFUSED
			: (status & k_compress_status_not_finite) != 0 ? ACLHIP_COMPRESS_NOT_FINITE : ACLHIP_COMPRESS_NOT_NORMALIZED;
		launch.results[instance] = make_uint2(result, 0);
		if (result == ACLHIP_COMPRESS_REFUSED)
			atomicAdd(launch.rejected_count, 1ull);
	}

	// The header words every transform blob has alike: raw_buffer_header (the hash is compress_hash_kernel's), tracks_header up to the
	// sample rate, and of transform_tracks_header the six counts and "no database". One lane's.
	__device__ __forceinline__ void transform_compress_write_common_header(uint32_t* words, uint32_t size, uint32_t num_tracks, uint32_t num_samples, float sample_rate,
		const uint32_t (&num_animated)[3], const uint32_t (&num_constant)[3])
	{
		words[0] = size;
		words[1] = 0;
		words[2] = k_tag_compressed_tracks;
		words[3] = uint32_t(k_version_latest) | (uint32_t(k_algorithm_uniformly_sampled) << 16) | (uint32_t(k_track_type_qvvf) << 24);
		words[4] = num_tracks;
		words[5] = num_samples;
		words[6] = __float_as_uint(sample_rate);
		words[10] = num_animated[0];
		words[11] = num_animated[1];
		words[12] = num_animated[2];
		words[13] = num_constant[0];
		words[14] = num_constant[1];
		words[15] = num_constant[2];
		words[16] = k_invalid_offset;
	}

	// A constant drop-w rotation, the `rank`-th of `num_constant`, into the constant rotations at `section` (write_stream_data.h:213-267):
	// groups of four as xxxx yyyy zzzz, a last group of n as n, n and n; normalized and of positive w
	__device__ __forceinline__ void transform_compress_write_constant_rotation(uint32_t* section, const uint32_t* in, uint32_t rank, uint32_t num_constant)
	{
		const float4 rotation = tracks_compress_positive_w(tracks_compress_normalize(*reinterpret_cast<const f32x4*>(in)));
		const uint32_t group = rank / 4u, entry = rank % 4u, group_size = num_constant - group * 4u < 4u ? num_constant - group * 4u : 4u;
		uint32_t* out = section + group * 12u;
		out[entry] = __float_as_uint(rotation.x);
		out[group_size + entry] = __float_as_uint(rotation.y);
		out[2u * group_size + entry] = __float_as_uint(rotation.z);
	}

	// The metadata of a blob with parents (write_track_metadata.h:106-194) at `metadata_at`: the parent indices as output indices, the
	// descriptions, the optional_metadata_header. The whole wave's.
	__device__ __forceinline__ void transform_compress_write_tail(const transform_compress_launch& launch, uint8_t* blob, uint64_t metadata_at, uint32_t num_tracks, uint32_t lane, bool with_descriptions)
	{
		uint32_t* tail = reinterpret_cast<uint32_t*>(blob + metadata_at);
		for (uint32_t track = lane; track < num_tracks; track += k_wave_size)
			tail[track] = compress_track_parent(launch, track, num_tracks);
		uint32_t* descriptions = tail + num_tracks;
		if (with_descriptions)
		{
			// precision, shell distance, the default rotation xyzw, translation xyz, scale xyz
			const uint32_t* default_pose = reinterpret_cast<const uint32_t*>(launch.default_pose);
			for (uint32_t word = lane; word < num_tracks * 12u; word += k_wave_size)
			{
				const uint32_t track = word / 12u, field = word - track * 12u;
				uint32_t value;
				if (field == 0)
					value = __float_as_uint(compress_track_precision(launch, track));
				else if (field == 1)
					value = __float_as_uint(compress_track_shell_distance(launch, track));
				else
				{
					const uint32_t at = field - 2u;			// 0 .. 9 -> QVV48 dwords 0 1 2 3 | 4 5 6 | 8 9 10; the identity: w and the scale are 1
					value = default_pose != nullptr ? default_pose[size_t(track) * 12u + at + (at >= 7u ? 1u : 0u)] : (at == 3u || at >= 7u) ? 0x3F800000u : 0u;
				}
				descriptions[word] = value;
			}
			descriptions += size_t(num_tracks) * 12u;
		}
		if (lane < 5)
		{
			// optional_metadata_header: no list name, no track names, parent indices, track descriptions, no contributing error
			const uint32_t offset = lane == 2 ? uint32_t(metadata_at) : lane == 3 && with_descriptions ? uint32_t(metadata_at) + 4u * num_tracks : k_invalid_offset;
			descriptions[lane] = offset;
		}
	}

	// ---- per instance: the statuses, where everything goes, and everything but the stream -------------------------------------------------------
	// One wave64 per instance, lanes <-> tracks, 64 at a time. A first pass over the flag bytes gives the statuses, the three constant and
	// the three animated counts and has_scale, and with them the size -- and the refusal against the stride, in front of any write to the
	// row. A second pass gives every track its place: a constant sub-track's in the constant data (rotations, then translations, then scales:
	// write_stream_data.h:199-310), an animated one's in its type's list, its type's in the packed words (write_sub_track_types.h). Then the
	// headers (compress.transform.impl.h:404-452, write_segment_data.h:67-122), the metadata (write_track_metadata.h:106-194) or the tail.
	// kDropW (aclhip_compress_tracks_batch with quatf_drop_w_full): the statuses, the sample count behind the looping vote and the wrap bit
	// are tracks_compress_shell_kernel's, in the instance's record; a rotation is three words, normalized and of positive w.
	template<bool kDropW>
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void transform_compress_layout_kernel(transform_compress_launch launch)
	{
		constexpr uint32_t rotation_width = kDropW ? 3u : 4u;
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t instance = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		if (instance >= launch.num_instances)
			return;

		const uint32_t handle = as_constant(launch.raws)[instance];
		const device_raw_tracks raw = load_raw_tracks_fields(launch.arrays, handle < launch.num_arrays ? handle : 0);
		const uint32_t num_tracks = raw.num_tracks;
		uint32_t num_samples = raw.num_samples;
		const uint8_t* track_flags = launch.track_flags + size_t(instance) * launch.max_tracks;

		compress_instance record = {};
		uint32_t status = transform_compress_refused(launch, handle, raw) ? k_compress_status_refused : 0u;
		uint32_t wrap = raw.looping_policy == k_loop_wrap ? 1u : 0u;
		if constexpr (kDropW)
		{
			const compress_instance voted = load_compress_instance(launch.instances, instance);
			status = voted.status;
			num_samples = voted.num_out_samples;
			wrap = voted.wrap;
		}
		uint32_t num_constant[3] = { 0, 0, 0 }, num_animated[3] = { 0, 0, 0 };
		if (status == 0)
		{
			for (uint32_t first = 0; first < num_tracks; first += k_wave_size)
			{
				const uint32_t flags = first + lane < num_tracks ? track_flags[first + lane] : 0u;
				status |= __ballot((flags & k_transform_flag_not_finite) != 0) != 0 ? k_compress_status_not_finite : 0u;
				status |= __ballot((flags & k_transform_flag_not_normalized) != 0) != 0 ? k_compress_status_not_normalized : 0u;
				#pragma unroll
				for (uint32_t kind = 0; kind < 3; ++kind)
				{
					const uint32_t type = (flags >> (2u * kind)) & 3u;
					num_constant[kind] += uint32_t(__popcll(__ballot(type == k_sub_track_constant)));
					num_animated[kind] += uint32_t(__popcll(__ballot(type == k_sub_track_animated)));
				}
			}
		}

		const bool has_scale = num_constant[2] + num_animated[2] != 0;
		const bool with_descriptions = (launch.flags & k_compress_include_descriptions) != 0;
		const bool with_parents = with_descriptions || (launch.flags & k_compress_include_parents) != 0;
		const uint32_t type_words = (num_tracks + 15u) / 16u;
		const uint32_t types_bytes = 4u * type_words * (has_scale ? 3u : 2u);
		const uint32_t constant_bytes = 4u * rotation_width * num_constant[0] + 12u * num_constant[1] + 12u * num_constant[2];
		const uint32_t pose_dwords = rotation_width * num_animated[0] + 3u * num_animated[1] + 3u * num_animated[2];
		const uint64_t stream_bytes = 4ull * pose_dwords * num_samples;
		const uint32_t constants_at = k_transform_blob_headers + types_bytes;
		const uint32_t stream_at = constants_at + constant_bytes;
		const uint64_t metadata_at = stream_at + stream_bytes;
		const uint64_t size = metadata_at + (with_parents ? 4ull * num_tracks + (with_descriptions ? 48ull * num_tracks : 0ull) + sizeof(optional_metadata_header) : 15ull);
		// (a blob's size is a 32 bit field; the reference counts the stream's bits in 32 bits)
		if (status == 0 && (size > launch.blob_stride_bytes || size > 0xFFFFFFFFull || stream_bytes * 8u > 0xFFFFFFFFull))
			status = k_compress_status_refused;

		if (status != 0)
		{
			if (lane == 0)
			{
				record.status = status;
				launch.instances[instance] = record;
				compress_write_refusal(launch, instance, status);
			}
			return;
		}

		uint8_t* blob = launch.blobs + uint64_t(instance) * launch.blob_stride_bytes;
		if (lane == 0)
		{
			record.samples = reinterpret_cast<const float*>(raw.samples);
			record.num_tracks = num_tracks;
			record.num_samples = record.num_out_samples = num_samples;
			record.track_type = k_track_type_qvvf;
			record.wrap = wrap;
			record.sample_rate = raw.sample_rate;
			record.size = uint32_t(size);
			record.num_bits_per_frame = pose_dwords * 32u;
			record.num_animated = num_animated[0];
			record.animated_offset = stream_at;
			record.num_animated_translations = num_animated[1];
			record.num_animated_scales = num_animated[2];
			launch.instances[instance] = record;
			launch.results[instance] = make_uint2(ACLHIP_COMPRESS_OK, uint32_t(size));

			uint32_t* words = reinterpret_cast<uint32_t*>(blob);
			transform_compress_write_common_header(words, uint32_t(size), num_tracks, num_samples, raw.sample_rate, num_animated, num_constant);
			// has_scale | default scale 1 (0 for an additive1 clip) | the three full formats (0) | no database, no trivial defaults (quat_near_identity with a
			// threshold of 0 holds for no rotation), no stripped key frames | wrap optimized | metadata
			words[7] = (has_scale ? 1u : 0u) | transform_compress_default_scale_bit(launch) | (kDropW ? uint32_t(k_rotation_quatf_drop_w_full) << 4 : 0u) | (record.wrap != 0 ? 1u << 30 : 0u) | (with_parents ? 1u << 31 : 0u);
			words[8] = 1;								// transform_tracks_header: one segment; offsets from its own start
			words[9] = 0;								// no variable sub-tracks
			words[17] = uint32_t(sizeof(transform_tracks_header));
			words[18] = k_transform_blob_headers - k_transform_header_offset;
			words[19] = constants_at - k_transform_header_offset;
			words[20] = stream_at - k_transform_header_offset;		// no clip range data
			words[21] = pose_dwords * 32u;				// segment_header
			words[22] = num_animated[0] * (32u * rotation_width);
			words[23] = num_animated[1] * 96u;
			words[24] = stream_at - k_transform_header_offset;		// no format per track data, no segment range data
		}

		// every track's place
		const uint32_t* first_frame = reinterpret_cast<const uint32_t*>(raw.samples);
		uint16_t* animated = launch.animated + size_t(instance) * 3u * launch.max_tracks;
		uint32_t constants_before[3] = { 0, 0, 0 }, animated_before[3] = { 0, 0, 0 };
		const uint32_t section_at[3] = { constants_at, constants_at + 4u * rotation_width * num_constant[0], constants_at + 4u * rotation_width * num_constant[0] + 12u * num_constant[1] };
		for (uint32_t first = 0; first < num_tracks; first += k_wave_size)
		{
			const uint32_t track = first + lane;
			const uint32_t flags = track < num_tracks ? track_flags[track] : 0u;
			#pragma unroll
			for (uint32_t kind = 0; kind < 3; ++kind)
			{
				const uint32_t type = (flags >> (2u * kind)) & 3u;
				const uint32_t width = kind == 0 ? rotation_width : 3u;
				const uint64_t constant_mask = __ballot(type == k_sub_track_constant), animated_mask = __ballot(type == k_sub_track_animated);
				if (type == k_sub_track_constant)
				{
					uint32_t* out = reinterpret_cast<uint32_t*>(blob + section_at[kind]) + (constants_before[kind] + transform_compress_rank(constant_mask)) * width;
					const uint32_t* in = first_frame + size_t(track) * 12u + kind * 4u;
					if (kDropW && kind == 0)
						transform_compress_write_constant_rotation(reinterpret_cast<uint32_t*>(blob + section_at[0]), in, constants_before[0] + transform_compress_rank(constant_mask), num_constant[0]);
					else
						for (uint32_t component = 0; component < width; ++component)
							out[component] = in[component];
				}
				if (type == k_sub_track_animated)
					animated[kind * launch.max_tracks + animated_before[kind] + transform_compress_rank(animated_mask)] = uint16_t(track);
				constants_before[kind] += uint32_t(__popcll(constant_mask));
				animated_before[kind] += uint32_t(__popcll(animated_mask));

				const uint32_t packed = transform_compress_pack_types(type, lane);
				if ((kind < 2 || has_scale) && (lane & 15u) == 0 && track < num_tracks)
					reinterpret_cast<uint32_t*>(blob + k_transform_blob_headers)[kind * type_words + track / 16u] = packed;
			}
		}

		uint32_t* tail = reinterpret_cast<uint32_t*>(blob + metadata_at);
		if (!with_parents)
		{
			// 15 zero bytes: three dwords and three bytes; nothing behind `size` is touched
			if (lane < 3)
				tail[lane] = 0;
			else if (lane < 6)
				blob[metadata_at + 9u + lane] = 0;
			return;
		}
		transform_compress_write_tail(launch, blob, metadata_at, num_tracks, lane, with_descriptions);
	}

	// ---- the animated stream ----------------------------------------------------------------------------------------------------------------
	// A lane owns one DWORD of the stream (write_stream_data.h:312-458 with full formats: per sample, the animated rotations xyzw, then the
	// translations xyz, then the scales xyz, each in track order; every float as a 32 bit word, most significant byte first). The pose is a
	// whole number of dwords: a division gives the sample and the slot, compares give the type, the list gives the track. One 4 byte load,
	// a byte swap, one coalesced store; no atomics and no zero fill.
	// kDropW: a rotation is x, y, z of the registered sample normalized and made of positive w -- a rotation's lane loads the whole quaternion.
	template<bool kDropW>
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void transform_compress_stream_kernel(transform_compress_launch launch)
	{
		constexpr uint32_t rotation_width = kDropW ? 3u : 4u;
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t wave = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		const uint32_t instance = wave / launch.waves_per_instance;
		const uint32_t share = wave - instance * launch.waves_per_instance;
		if (instance >= launch.num_instances)
			return;

		const compress_instance record = load_compress_instance(launch.instances, instance);
		if (record.status != 0)
			return;

		const uint32_t rotation_dwords = record.num_animated * rotation_width;
		const uint32_t translation_dwords = record.num_animated_translations * 3u;
		const uint32_t pose_dwords = record.num_bits_per_frame / 32u;
		const uint32_t num_dwords = pose_dwords * record.num_samples;		// < 2^27 (layout refuses the rest)
		const uint32_t* samples = reinterpret_cast<const uint32_t*>(record.samples);
		const uint16_t* animated = launch.animated + size_t(instance) * 3u * launch.max_tracks;
		uint32_t* out = reinterpret_cast<uint32_t*>(launch.blobs + uint64_t(instance) * launch.blob_stride_bytes + record.animated_offset);

		for (uint32_t dword = share * k_wave_size + lane; dword < num_dwords; dword += launch.waves_per_instance * k_wave_size)
		{
			const uint32_t sample = dword / pose_dwords;
			uint32_t slot = dword - sample * pose_dwords;
			uint32_t kind = 0, width = rotation_width;
			if (slot >= rotation_dwords)
			{
				slot -= rotation_dwords;
				kind = 1;
				width = 3;
				if (slot >= translation_dwords)
				{
					slot -= translation_dwords;
					kind = 2;
				}
			}
			const uint32_t entry = slot / width, component = slot - entry * width;
			const uint32_t track = animated[kind * launch.max_tracks + entry];
			if constexpr (kDropW)
			{
				const uint32_t* in = samples + (size_t(sample) * record.num_tracks + track) * 12u + kind * 4u;
				uint32_t value;
				if (kind == 0)
				{
					const float4 rotation = tracks_compress_positive_w(tracks_compress_normalize(*reinterpret_cast<const f32x4*>(in)));
					value = __float_as_uint(component == 0 ? rotation.x : component == 1 ? rotation.y : rotation.z);
				}
				else
					value = in[component];
				out[dword] = __builtin_bswap32(value);
			}
			else
				out[dword] = __builtin_bswap32(samples[(size_t(sample) * record.num_tracks + track) * 12u + kind * 4u + component]);
		}
	}
