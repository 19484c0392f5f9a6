// kernels_scalar_compress.inl -- part of aclhip.hip (one translation unit; included there behind kernels_raw_scalar_tracks.inl, not compiled on its own).
// aclhip_compress_raw_scalar_tracks_batch: acl::compress_track_list for float1f .. vector4f (compression/impl/compress.scalar.impl.h:65-269
// and the files it calls) over a batch of raw scalar track arrays, in five stream ordered launches -- the data dependences set the cuts:
//   scalar_compress_prepare_kernel   per instance: handle, record, refusal, the looping vote (2 key frames)
//   scalar_compress_analyze_kernel   per (instance, track): the finite check, ranges with the reference's tie rule, constant test, rate search
//   scalar_compress_layout_kernel    per instance: prefix sums over the tracks, the size, the refusal against the stride, headers,
//                                    per-track metadata, constant and range values
//   scalar_compress_write_kernel     per output dword of the animated bit stream (and of the tail behind it): a lane gathers the values that
//                                    fall into its dword -- no atomics, the same bytes on every run
//   compress_hash_kernel             per instance: FNV-1a 32 over [8, size), serial in the bytes; the wave stages the loads, the chain runs
//                                    on the scalar unit
// include/aclhip.h states the definition (fp32, one IEEE operation at a time: this file is compiled with -ffp-contract=off; the division is
// the compiler's correctly rounded one -- nothing is proven about a caller's values, so none of the clip decode's short forms is used).

	// What the launches hand to each other, in the caller's workspace: one record per instance, one per (instance, track) and one per
	// (instance, animated track). Every byte that is read was written by an earlier launch of the same call. The record per instance is
	// the transform compressor's too (kernels_transform_compress.inl), and what compress_hash_kernel reads of either: status and size.
	struct compress_instance
	{
		const float* samples;
		uint32_t num_tracks;
		uint32_t num_samples;			// as registered: the finite check covers the sample the vote may drop
		uint32_t num_out_samples;		// behind the vote
		uint32_t num_components;
		uint32_t track_type;
		uint32_t wrap;					// the blob is wrap optimized
		float sample_rate;
		uint32_t status;				// bit 0: a sample is not finite (analyze, atomic OR); bit 1: refused (prepare or layout)
		uint32_t size;					// layout: the blob's
		uint32_t num_bits_per_frame;
		// layout: what each compressor's stream kernel needs. (One flat record with a name for every word, not a union of a view per
		// compressor: with a union of any shape in this record the compiler orders the loads of the scalar analyze, layout and write
		// kernels differently.)
		uint32_t num_animated;					// scalar: tracks with bits in the stream; transform: animated rotations
		uint32_t animated_offset;				// of the stream, from the blob's start (4 byte aligned)
		uint32_t num_animated_translations;		// the transform compressor's; the scalar one leaves both 0
		uint32_t num_animated_scales;
	};
	static_assert(sizeof(compress_instance) == 64, "four dwordx4 loads");

	struct scalar_compress_track
	{
		float min[4];
		float extent[4];
		uint32_t rate;					// 0: constant; 1 .. 23; 24: raw
		uint32_t section_offset;		// layout: floats in front of this track in the constant section (rate 0) or in the range section (1 .. 23)
		uint32_t reserved[2];
	};
	static_assert(sizeof(scalar_compress_track) == 48, "workspace layout");

	struct scalar_compress_animated
	{
		uint32_t bit_offset;			// inside a frame; strictly ascending over an instance's entries
		uint32_t track_and_rate;		// track | rate << 24
	};

	constexpr uint32_t k_compress_status_not_finite = 1;
	constexpr uint32_t k_compress_status_refused = 2;
	constexpr uint32_t k_compress_raw_rate = 24;

	struct scalar_compress_launch
	{
		const device_raw_scalar_tracks* arrays;		// the context's raw scalar track table
		uint32_t num_arrays;
		uint32_t num_instances;
		const uint32_t* raws;						// [num_instances] handles
		const float* track_precisions;				// [num_track_precisions] or null
		uint32_t num_track_precisions;
		float precision;
		uint32_t optimize_loops;
		uint32_t max_tracks;
		compress_instance* instances;				// [num_instances]
		scalar_compress_track* tracks;				// [num_instances][max_tracks]
		scalar_compress_animated* animated;			// [num_instances][max_tracks]
		uint8_t* blobs;
		uint64_t blob_stride_bytes;
		uint2* results;								// [num_instances] aclhip_compress_result
		uint32_t waves_per_instance;				// the write kernel's
		unsigned long long* rejected_count;
	};

	// compress_hash_kernel's, filled in by both compressors
	struct compress_hash_launch
	{
		const compress_instance* instances;			// [num_instances]
		uint32_t num_instances;
		uint8_t* blobs;
		uint64_t blob_stride_bytes;
	};

	constexpr uint32_t k_compress_waves_per_block = 4;
	constexpr uint32_t k_compress_dwords_per_lane = 16;		// the output dwords one lane of the write kernel takes in turn, at most
	constexpr uint32_t k_compress_cached_values = 4;		// (sample, component) values per lane the rate search keeps normalized in registers

	__device__ __forceinline__ compress_instance load_compress_instance(const compress_instance* table, uint32_t index)
	{
		const ACLHIP_CONSTANT u32x4* source = (const ACLHIP_CONSTANT u32x4*)(table + index);
		struct { u32x4 a, b, c, d; } raw = { source[0], source[1], source[2], source[3] };
		compress_instance instance;
		__builtin_memcpy(&instance, &raw, sizeof(instance));
		return instance;
	}

	__device__ __forceinline__ float compress_precision_of(const scalar_compress_launch& launch, uint32_t track)
	{
		return launch.track_precisions != nullptr ? launch.track_precisions[track] : launch.precision;
	}

	__device__ __forceinline__ uint32_t compress_num_bits_at(uint32_t rate) { return rate == k_compress_raw_rate ? 32u : rate; }

	// normalize.scalar.h:44-76: (x - min) / extent, min(n, 1) with the second operand taken unless n < 1, 0 where the extent is (nearly) 0
	__device__ __forceinline__ float compress_normalize(float x, float range_min, float range_extent)
	{
		float n = (x - range_min) / range_extent;
		n = n < 1.0f ? n : 1.0f;
		return range_extent < 0.000000001f ? 0.0f : n;
	}

	// pack_vector4_uXX (quantize.scalar.h:75-82): round_symmetric of a value that is never negative
	__device__ __forceinline__ float compress_pack(float n, float max_value) { return floorf(n * max_value + 0.5f); }

	// one sample at one rate (quantize.scalar.h:116-132): decay, undo the normalization as a multiply and an add, compare
	__device__ __forceinline__ bool compress_rate_passes(float x, float n, float range_min, float range_extent, float max_value, float inv_max_value, float precision)
	{
		const float decayed = compress_pack(n, max_value) * inv_max_value;
		const float restored = decayed * range_extent + range_min;
		return fabsf(x - restored) <= precision;
	}

	__device__ __forceinline__ float compress_select(const float (&values)[4], uint32_t component)
	{
		return component == 0 ? values[0] : component == 1 ? values[1] : component == 2 ? values[2] : values[3];
	}

	// ---- per instance: handle, record, refusal, the looping vote -----------------------------------------------------------------------------
	// One wave64 per instance. The scalar unit reads the handle and the record and decides the refusal in front of any load of a sample
	// (sample_raw_scalar_tracks_kernel's prologue); the lanes take the T * C elements of the first and the last key frame for the vote
	// (optimize_looping.scalar.h:59-79: every track and component within its track's precision, or nothing is dropped).
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void scalar_compress_prepare_kernel(scalar_compress_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t instance = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		if (instance >= launch.num_instances)
			return;

		const uint32_t handle = as_constant(launch.raws)[instance];
		const device_raw_scalar_tracks raw = load_raw_scalar_tracks_fields(launch.arrays, handle < launch.num_arrays ? handle : 0);
		const uint32_t num_tracks = raw.num_tracks;
		const uint32_t num_components = raw.num_components;
		const uint32_t num_samples = raw.num_samples;

		compress_instance record = {};
		const bool refused = handle >= launch.num_arrays || raw.samples == nullptr || num_tracks > launch.max_tracks
			|| (launch.track_precisions != nullptr && num_tracks > launch.num_track_precisions);
		if (refused)
		{
			if (lane == 0)
			{
				record.status = k_compress_status_refused;
				launch.instances[instance] = record;
				launch.results[instance] = make_uint2(ACLHIP_COMPRESS_REFUSED, 0);
				atomicAdd(launch.rejected_count, 1ull);
			}
			return;
		}

		bool wrap = raw_scalar_looping_policy_of(raw) == k_loop_wrap;
		uint32_t num_out_samples = num_samples;
		if (!wrap && launch.optimize_loops != 0 && num_samples > 1)
		{
			const uint32_t num_elements = num_tracks * num_components;
			const float* first = raw.samples;
			const float* last = raw.samples + size_t(num_samples - 1) * num_elements;
			bool near = true;
			for (uint32_t element = lane; element < num_elements; element += k_wave_size)
			{
				const float precision = compress_precision_of(launch, raw_scalar_track_of(element, num_components));
				near = near && fabsf(first[element] - last[element]) <= precision;
			}
			if (__ballot(!near) == 0)
			{
				wrap = true;
				num_out_samples = num_samples - 1;
			}
		}

		if (lane == 0)
		{
			record.samples = raw.samples;
			record.num_tracks = num_tracks;
			record.num_samples = num_samples;
			record.num_out_samples = num_out_samples;
			record.num_components = num_components;
			record.track_type = raw_scalar_track_type_of(raw);
			record.wrap = wrap ? 1u : 0u;
			record.sample_rate = raw.sample_rate;
			launch.instances[instance] = record;
		}
	}

	// The reference's sequential minimum (track_range_impl.h:54-59: min = min < x ? min : x from 1e10, in ascending sample order) has the
	// VALUE of the smallest operand, the start included, and the BITS of the last operand equal to it -- +0 and -0 compare equal, so the
	// sign of a zero extreme is that of the last zero. A lane keeps (value, sample index of the last equal operand; -1: the start) over its
	// own samples in ascending order with the reference's own comparison, and the wave combines pairs: the smaller value, the later index
	// on a tie. The maximum is the same with the comparison turned round.
	template<bool kMinimum>
	__device__ __forceinline__ void compress_extreme_step(float& extreme, int32_t& at, float x, int32_t sample)
	{
		const bool keep = kMinimum ? extreme < x : extreme > x;
		extreme = keep ? extreme : x;
		at = keep ? at : sample;
	}

	template<bool kMinimum>
	__device__ __forceinline__ float compress_wave_extreme(float extreme, int32_t at)
	{
		#pragma unroll
		for (int offset = int(k_wave_size) / 2; offset != 0; offset >>= 1)
		{
			const float other = __shfl_xor(extreme, offset);
			const int32_t other_at = __shfl_xor(at, offset);
			const bool other_wins = kMinimum ? other < extreme : other > extreme;
			const bool mine_wins = kMinimum ? extreme < other : extreme > other;
			const bool take = other_wins || (!mine_wins && other_at > at);
			extreme = take ? other : extreme;
			at = take ? other_at : at;
		}
		return extreme;
	}

	// ---- per (instance, track): finite check, ranges, constant test, rate search ---------------------------------------------------------------
	// One wave64 per track, samples across the lanes (a track's samples lie T * C floats apart: the four waves of a block take neighbouring
	// tracks and share the lines). blockIdx.y walks the instances.
	//   finite    every float of the track over the REGISTERED samples; one hit marks the instance and ends the wave
	//   ranges    per component, over the samples behind the vote
	//   constant  |extent[c]| < precision for every component, strictly
	//   search    rates 23 .. 1, ended by the first that fails (wave uniform: the reference's own loop). A lane keeps its first
	//             k_compress_cached_values values and their normalized forms in registers -- S * C <= 256 divides once per value --, and
	//             recomputes what lies beyond per rate
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void scalar_compress_analyze_kernel(scalar_compress_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t track = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		for (uint32_t instance = blockIdx.y; instance < launch.num_instances; instance += gridDim.y)
		{
			const compress_instance record = load_compress_instance(launch.instances, instance);
			if ((record.status & k_compress_status_refused) != 0 || track >= record.num_tracks)
				continue;

			const uint32_t num_components = record.num_components;
			const uint32_t num_samples = record.num_samples;
			const uint32_t num_out_samples = record.num_out_samples;
			const size_t row = size_t(record.num_tracks) * num_components;
			const float* base = record.samples + size_t(track) * num_components;
			const float precision = compress_precision_of(launch, track);

			float range_min[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, range_extent[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
			bool finite = true;
			#pragma unroll
			for (uint32_t component = 0; component < 4; ++component)
			{
				if (component < num_components)
				{
					float lowest = 1.0e10f, highest = -1.0e10f;
					int32_t lowest_at = -1, highest_at = -1;
					for (uint32_t sample = lane; sample < num_samples; sample += k_wave_size)
					{
						const float x = base[sample * row + component];
						finite = finite && (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u;
						if (sample < num_out_samples)
						{
							compress_extreme_step<true>(lowest, lowest_at, x, int32_t(sample));
							compress_extreme_step<false>(highest, highest_at, x, int32_t(sample));
						}
					}
					lowest = compress_wave_extreme<true>(lowest, lowest_at);
					highest = compress_wave_extreme<false>(highest, highest_at);
					range_min[component] = lowest;
					range_extent[component] = highest - lowest;
				}
			}
			if (__ballot(!finite) != 0)
			{
				if (lane == 0)
					atomicOr(&launch.instances[instance].status, k_compress_status_not_finite);
				continue;
			}

			bool constant = true;
			#pragma unroll
			for (uint32_t component = 0; component < 4; ++component)
				constant = constant && (component >= num_components || fabsf(range_extent[component]) < precision);

			uint32_t best = k_compress_raw_rate;
			if (!constant)
			{
				const uint32_t num_values = num_out_samples * num_components;		// (sample, component) pairs of the track, sample major
				float xs[k_compress_cached_values], ns[k_compress_cached_values], mins[k_compress_cached_values], extents[k_compress_cached_values];
				#pragma unroll
				for (uint32_t k = 0; k < k_compress_cached_values; ++k)
				{
					const uint32_t value = lane + k * k_wave_size;
					xs[k] = ns[k] = mins[k] = extents[k] = 0.0f;
					if (value < num_values)
					{
						const uint32_t sample = raw_scalar_track_of(value, num_components);		// value / C
						const uint32_t component = value - sample * num_components;
						mins[k] = compress_select(range_min, component);
						extents[k] = compress_select(range_extent, component);
						xs[k] = base[sample * row + component];
						ns[k] = compress_normalize(xs[k], mins[k], extents[k]);
					}
				}

				for (uint32_t rate = k_compress_raw_rate - 1; rate != 0; --rate)
				{
					const float max_value = float((1u << rate) - 1u);
					const float inv_max_value = 1.0f / max_value;
					bool passes = true;
					#pragma unroll
					for (uint32_t k = 0; k < k_compress_cached_values; ++k)
						passes = passes && (lane + k * k_wave_size >= num_values || compress_rate_passes(xs[k], ns[k], mins[k], extents[k], max_value, inv_max_value, precision));
					bool failed = __ballot(!passes) != 0;
					for (uint32_t first = k_compress_cached_values * k_wave_size; first < num_values && !failed; first += k_wave_size)
					{
						const uint32_t value = first + lane;
						if (value < num_values)
						{
							const uint32_t sample = raw_scalar_track_of(value, num_components);
							const uint32_t component = value - sample * num_components;
							const float lowest = compress_select(range_min, component), extent = compress_select(range_extent, component);
							const float x = base[sample * row + component];
							passes = compress_rate_passes(x, compress_normalize(x, lowest, extent), lowest, extent, max_value, inv_max_value, precision);
						}
						failed = __ballot(!passes) != 0;
					}
					if (failed)
						break;
					best = rate;
				}
			}

			if (lane == 0)
			{
				scalar_compress_track out = {};
				#pragma unroll
				for (uint32_t component = 0; component < 4; ++component)
				{
					out.min[component] = range_min[component];
					out.extent[component] = range_extent[component];
				}
				out.rate = constant ? 0u : best;
				launch.tracks[size_t(instance) * launch.max_tracks + track] = out;
			}
		}
	}

	__device__ __forceinline__ uint32_t compress_wave_inclusive_scan(uint32_t value, uint32_t lane)
	{
		#pragma unroll
		for (uint32_t offset = 1; offset < k_wave_size; offset <<= 1)
		{
			const uint32_t other = uint32_t(__shfl_up(int(value), offset));
			value += lane >= offset ? other : 0u;
		}
		return value;
	}

	// ---- per instance: where everything goes, and everything but the stream -------------------------------------------------------------------
	// One wave64 per instance, lanes <-> tracks, 64 at a time with running totals: a track's place in the constant or in the range section, an
	// animated track's entry (its bit offset inside a frame) in the instance's compact list. Then the size -- and the refusal against the
	// stride, in front of any write to the row --, the three headers (compress.scalar.impl.h:143-175), one rate byte per track with its
	// padding, sample 0 of the constant tracks and (min, extent) of the quantized ones (write_track_data_impl.h:46-130).
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void scalar_compress_layout_kernel(scalar_compress_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t instance = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		if (instance >= launch.num_instances)
			return;

		const compress_instance record = load_compress_instance(launch.instances, instance);
		if ((record.status & k_compress_status_refused) != 0)
			return;		// (prepare said so)
		if ((record.status & k_compress_status_not_finite) != 0)
		{
			if (lane == 0)
				launch.results[instance] = make_uint2(ACLHIP_COMPRESS_NOT_FINITE, 0);
			return;
		}

		const uint32_t num_tracks = record.num_tracks;
		const uint32_t num_components = record.num_components;
		scalar_compress_track* tracks = launch.tracks + size_t(instance) * launch.max_tracks;
		scalar_compress_animated* animated = launch.animated + size_t(instance) * launch.max_tracks;

		uint32_t constant_floats = 0, range_floats = 0, frame_bits = 0, num_animated = 0;
		for (uint32_t first = 0; first < num_tracks; first += k_wave_size)
		{
			const uint32_t track = first + lane;
			const bool valid = track < num_tracks;
			const uint32_t rate = valid ? tracks[track].rate : 0u;
			const uint32_t own_constant = valid && rate == 0 ? num_components : 0u;
			const uint32_t own_range = valid && rate != 0 && rate != k_compress_raw_rate ? 2u * num_components : 0u;
			const uint32_t own_bits = valid && rate != 0 ? compress_num_bits_at(rate) * num_components : 0u;
			const uint32_t own_animated = own_bits != 0 ? 1u : 0u;
			const uint32_t scan_constant = compress_wave_inclusive_scan(own_constant, lane);
			const uint32_t scan_range = compress_wave_inclusive_scan(own_range, lane);
			const uint32_t scan_bits = compress_wave_inclusive_scan(own_bits, lane);
			const uint32_t scan_animated = compress_wave_inclusive_scan(own_animated, lane);
			if (valid)
				tracks[track].section_offset = rate == 0 ? constant_floats + scan_constant - own_constant : range_floats + scan_range - own_range;
			if (own_animated != 0)
				animated[num_animated + scan_animated - 1u] = scalar_compress_animated{ frame_bits + scan_bits - own_bits, track | (rate << 24) };
			constant_floats += uint32_t(__builtin_amdgcn_readlane(int(scan_constant), 63));
			range_floats += uint32_t(__builtin_amdgcn_readlane(int(scan_range), 63));
			frame_bits += uint32_t(__builtin_amdgcn_readlane(int(scan_bits), 63));
			num_animated += uint32_t(__builtin_amdgcn_readlane(int(scan_animated), 63));
		}

		const uint32_t metadata_bytes = align_to_u32(num_tracks, 4);
		const uint32_t constants_at = 52u + metadata_bytes;
		const uint64_t ranges_at = uint64_t(constants_at) + 4ull * constant_floats;
		const uint64_t animated_at = ranges_at + 4ull * range_floats;
		const uint64_t stream_bits = uint64_t(frame_bits) * record.num_out_samples;
		const uint64_t size = animated_at + (stream_bits + 7u) / 8u + 15u;
		// (a blob's size is a 32 bit field; the reference counts the stream's bits in 32 bits as well)
		if (size > launch.blob_stride_bytes || stream_bits > 0xFFFFFFFFull || size > 0xFFFFFFFFull)
		{
			if (lane == 0)
			{
				launch.instances[instance].status = k_compress_status_refused;
				launch.results[instance] = make_uint2(ACLHIP_COMPRESS_REFUSED, 0);
				atomicAdd(launch.rejected_count, 1ull);
			}
			return;
		}

		uint8_t* blob = launch.blobs + uint64_t(instance) * launch.blob_stride_bytes;
		if (lane == 0)
		{
			compress_instance* out = launch.instances + instance;
			out->size = uint32_t(size);
			out->num_bits_per_frame = frame_bits;
			out->num_animated = num_animated;
			out->animated_offset = uint32_t(animated_at);
			launch.results[instance] = make_uint2(ACLHIP_COMPRESS_OK, uint32_t(size));

			uint32_t* words = reinterpret_cast<uint32_t*>(blob);
			words[0] = uint32_t(size);					// raw_buffer_header; the hash is compress_hash_kernel's
			words[1] = 0;
			words[2] = k_tag_compressed_tracks;			// tracks_header
			words[3] = uint32_t(k_version_latest) | (uint32_t(k_algorithm_uniformly_sampled) << 16) | (record.track_type << 24);
			words[4] = num_tracks;
			words[5] = record.num_out_samples;
			words[6] = __float_as_uint(record.sample_rate);
			words[7] = record.wrap != 0 ? 1u << 30 : 0u;
			words[8] = frame_bits;						// scalar_tracks_header; offsets from its own start
			words[9] = uint32_t(sizeof(scalar_tracks_header));
			words[10] = constants_at - 32u;
			words[11] = uint32_t(ranges_at) - 32u;
			words[12] = uint32_t(animated_at) - 32u;
		}

		for (uint32_t byte = lane; byte < metadata_bytes; byte += k_wave_size)
			blob[52u + byte] = byte < num_tracks ? uint8_t(tracks[byte].rate) : uint8_t(0);

		const float* first_frame = record.samples;
		for (uint32_t track = lane; track < num_tracks; track += k_wave_size)		// (the lane that wrote the track's section_offset above)
		{
			const scalar_compress_track entry = tracks[track];
			if (entry.rate == 0)
			{
				float* out = reinterpret_cast<float*>(blob + constants_at) + entry.section_offset;
				for (uint32_t component = 0; component < num_components; ++component)
					out[component] = first_frame[size_t(track) * num_components + component];
			}
			else if (entry.rate != k_compress_raw_rate)
			{
				float* out = reinterpret_cast<float*>(blob + ranges_at) + entry.section_offset;
				for (uint32_t component = 0; component < num_components; ++component)
				{
					out[component] = entry.min[component];
					out[num_components + component] = entry.extent[component];
				}
			}
		}
	}

	// ---- the animated bit stream and the tail -------------------------------------------------------------------------------------------------
	// A lane owns one DWORD of [animated_offset, size): 32 bits of the stream (write_track_data_impl.h:132-189: per sample, per animated track,
	// per component, num_bits(rate) bits, most significant bit first), zero where the stream has ended -- the padding to a whole byte and the
	// 15 byte tail. It finds the frame and the bit offset inside it by a division, the track by a binary search over the instance's animated
	// entries, and walks the values that reach into its dword: a value that straddles two dwords is made by both lanes. The 1 to 3 bytes
	// behind the last whole dword are tail bytes and are stored one by one: nothing behind `size` is touched.
	__global__ __launch_bounds__(k_compress_waves_per_block * k_wave_size) void scalar_compress_write_kernel(scalar_compress_launch launch)
	{
		const uint32_t lane = threadIdx.x & (k_wave_size - 1);
		const uint32_t wave = blockIdx.x * k_compress_waves_per_block + __builtin_amdgcn_readfirstlane(threadIdx.x / k_wave_size);
		const uint32_t instance = wave / launch.waves_per_instance;
		const uint32_t share = wave - instance * launch.waves_per_instance;
		if (instance >= launch.num_instances)
			return;

		const compress_instance record = load_compress_instance(launch.instances, instance);
		if (record.status != 0)
			return;

		const uint32_t num_tracks = record.num_tracks;
		const uint32_t num_components = record.num_components;
		const uint32_t frame_bits = record.num_bits_per_frame;
		const uint32_t num_animated = record.num_animated;
		const uint64_t stream_bits = uint64_t(frame_bits) * record.num_out_samples;		// < 2^32 (layout refuses the rest)
		const scalar_compress_track* tracks = launch.tracks + size_t(instance) * launch.max_tracks;
		const scalar_compress_animated* animated = launch.animated + size_t(instance) * launch.max_tracks;
		uint8_t* out = launch.blobs + uint64_t(instance) * launch.blob_stride_bytes + record.animated_offset;
		const uint32_t num_bytes = record.size - record.animated_offset;
		const uint32_t num_dwords = num_bytes / 4u;

		for (uint32_t dword = share * k_wave_size + lane; dword <= num_dwords; dword += launch.waves_per_instance * k_wave_size)
		{
			if (dword == num_dwords)
			{
				for (uint32_t byte = num_dwords * 4u; byte < num_bytes; ++byte)
					out[byte] = 0;
				break;
			}

			const uint64_t first_bit = uint64_t(dword) * 32u;
			uint32_t word = 0;		// stream order: bit 31 is the dword's first bit
			if (first_bit < stream_bits)
			{
				const int32_t end = stream_bits - first_bit < 32u ? int32_t(stream_bits - first_bit) : 32;
				uint32_t frame = uint32_t(first_bit) / frame_bits;
				const uint32_t frame_offset = uint32_t(first_bit) - frame * frame_bits;

				// the last entry that starts at or in front of frame_offset
				uint32_t low = 0, high = num_animated - 1u;
				while (low < high)
				{
					const uint32_t middle = (low + high + 1u) / 2u;
					if (animated[middle].bit_offset <= frame_offset)
						low = middle;
					else
						high = middle - 1u;
				}
				uint32_t index = low;
				scalar_compress_animated entry = animated[index];
				uint32_t track = entry.track_and_rate & 0xFFFFFFu, rate = entry.track_and_rate >> 24, num_bits = compress_num_bits_at(rate);
				const uint32_t inside = frame_offset - entry.bit_offset;
				uint32_t component = inside / num_bits;
				int32_t at = -int32_t(inside - component * num_bits);		// where the value starts, from the dword's first bit

				while (at < end)
				{
					const float x = record.samples[(size_t(frame) * num_tracks + track) * num_components + component];
					uint32_t value = __float_as_uint(x);
					if (rate != k_compress_raw_rate)
					{
						const float n = compress_normalize(x, tracks[track].min[component], tracks[track].extent[component]);
						value = uint32_t(compress_pack(n, float((1u << rate) - 1u)));
					}
					const uint32_t aligned = value << (32u - num_bits);
					word |= at >= 0 ? aligned >> uint32_t(at) : aligned << uint32_t(-at);
					at += int32_t(num_bits);
					if (++component == num_components)
					{
						component = 0;
						if (++index == num_animated)
						{
							index = 0;
							++frame;
						}
						entry = animated[index];
						track = entry.track_and_rate & 0xFFFFFFu;
						rate = entry.track_and_rate >> 24;
						num_bits = compress_num_bits_at(rate);
					}
				}
			}
			reinterpret_cast<uint32_t*>(out)[dword] = __builtin_bswap32(word);
		}
	}

	// ---- the hash -----------------------------------------------------------------------------------------------------------------------------
	// FNV-1a 32 (core/hash.h:86-99) over [8, size): every byte's step needs the step before it, so a blob is one chain and the parallelism
	// of the launch is across blobs. One wave64 per blob: the lanes load 256 bytes at a time, the next piece in flight while the chain
	// walks the current one out of the lanes' registers (v_readlane) on the scalar unit.
	__device__ __forceinline__ uint32_t compress_hash_step(uint32_t hash, uint32_t byte) { return (hash ^ byte) * 16777619u; }

	__global__ __launch_bounds__(k_wave_size) void compress_hash_kernel(compress_hash_launch launch)
	{
		const uint32_t lane = threadIdx.x;
		const uint32_t instance = blockIdx.x;
		const compress_instance record = load_compress_instance(launch.instances, instance);
		if (record.status != 0)
			return;

		uint32_t* blob = reinterpret_cast<uint32_t*>(launch.blobs + uint64_t(instance) * launch.blob_stride_bytes);
		const uint32_t* words = blob + 2;
		const uint32_t num_bytes = record.size - 8u;
		const uint32_t num_words = (num_bytes + 3u) / 4u;		// (a row ends 16 byte aligned: the last word lies inside it)

		uint32_t hash = 2166136261u;
		uint32_t next = lane < num_words ? words[lane] : 0u;
		for (uint32_t first_byte = 0; first_byte < num_bytes; first_byte += k_wave_size * 4u)
		{
			const uint32_t current = next;
			const uint32_t next_word = first_byte / 4u + k_wave_size + lane;
			next = next_word < num_words ? words[next_word] : 0u;

			const uint32_t piece_bytes = min(num_bytes - first_byte, k_wave_size * 4u);
			if (piece_bytes == k_wave_size * 4u)
			{
				#pragma unroll 8
				for (uint32_t source = 0; source < k_wave_size; ++source)
				{
					const uint32_t word = uint32_t(__builtin_amdgcn_readlane(int(current), int(source)));
					hash = compress_hash_step(hash, word & 0xFFu);
					hash = compress_hash_step(hash, (word >> 8) & 0xFFu);
					hash = compress_hash_step(hash, (word >> 16) & 0xFFu);
					hash = compress_hash_step(hash, word >> 24);
				}
			}
			else
			{
				for (uint32_t byte = 0; byte < piece_bytes; ++byte)
				{
					const uint32_t word = uint32_t(__builtin_amdgcn_readlane(int(current), int(byte / 4u)));
					hash = compress_hash_step(hash, (word >> ((byte & 3u) * 8u)) & 0xFFu);
				}
			}
		}
		if (lane == 0)
			blob[1] = hash;
	}
