// host_transform_compress.inl -- part of aclhip.hip (one translation unit; included there behind host_scalar_compress.inl, not compiled on its own).
// Host side of the three transform compressors, aclhip_compress_raw_tracks_batch (kernels_transform_compress.inl),
// aclhip_compress_tracks_batch (kernels_tracks_compress.inl) and aclhip_compress_tracks_variable_batch (kernels_variable_compress.inl),
// and of the bit rate search, aclhip_find_bit_rates_batch (kernels_bit_rate_search.inl) and, with every level,
// aclhip_find_bit_rates_level_batch, and of the last three with the error metric as
// an argument (the _metric entry points: the metric is one more thing a call says of itself, and picks the instantiations of its phases):
// the sizes a caller needs, and one argument check, one workspace layout and one launch record for all -- the raw call is the drop-w
// call with the full formats, no shell and its own words; the variable call is it with its own kernels behind the shell, its rate
// table and three more parts of the workspace; the search is the variable call without rows, its table written, and four more parts;
// the search with the levels is the search with its own words, one more part and one more launch. The _additive entry points are
// the drop-w call, the variable call and the search with the levels with the additive base as one more thing a call says of itself:
// it picks the instantiations of the kernels the base enters, and its format goes into the launch record.
// What a call says of itself is its transform_compress_kind; what the smaller descs, the rate table, the written and the read ranges,
// the variable launch record and the grid of a wave per segment are is stated once each, in front of the check and of the calls.
// What they share with the scalar compressor -- the cap of a size, the common checks, the launches' shapes, their front and their list
// of phases -- is in host_scalar_compress.inl. include/aclhip.h states the definitions.

static_assert(sizeof(aclhip_transform_compress_desc) == 80, "header layout");
static_assert(offsetof(aclhip_transform_compress_desc, default_pose) == 8 && offsetof(aclhip_transform_compress_desc, num_table_tracks) == 40
	&& offsetof(aclhip_transform_compress_desc, shell_distance) == 48 && offsetof(aclhip_transform_compress_desc, workspace) == 56
	&& offsetof(aclhip_transform_compress_desc, reserved) == 64, "header layout");
static_assert(sizeof(aclhip_find_bit_rates_desc) == 96, "header layout");
static_assert(offsetof(aclhip_find_bit_rates_desc, default_pose) == 16 && offsetof(aclhip_find_bit_rates_desc, precision) == 48
	&& offsetof(aclhip_find_bit_rates_desc, workspace) == 56 && offsetof(aclhip_find_bit_rates_desc, shell_metadata) == 64
	&& offsetof(aclhip_find_bit_rates_desc, level) == 72 && offsetof(aclhip_find_bit_rates_desc, reserved) == 80, "header layout");
static_assert(sizeof(aclhip_additive_base) == 32 && offsetof(aclhip_additive_base, additive_format) == 8 && offsetof(aclhip_additive_base, reserved) == 16, "header layout");
static_assert(sizeof(aclhip_compress_tracks_desc) == 96, "header layout");
static_assert(offsetof(aclhip_compress_tracks_desc, flags) == 12 && offsetof(aclhip_compress_tracks_desc, num_table_tracks) == 20
	&& offsetof(aclhip_compress_tracks_desc, default_pose) == 24 && offsetof(aclhip_compress_tracks_desc, track_shell_distances) == 48
	&& offsetof(aclhip_compress_tracks_desc, precision) == 56 && offsetof(aclhip_compress_tracks_desc, shell_distance) == 60
	&& offsetof(aclhip_compress_tracks_desc, workspace) == 64 && offsetof(aclhip_compress_tracks_desc, shell_metadata) == 72
	&& offsetof(aclhip_compress_tracks_desc, reserved) == 80, "header layout");

namespace
{
	constexpr uint32_t k_transform_compress_flags = ACLHIP_COMPRESS_OPTIMIZE_LOOPS | ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES | ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS;

	// What an entry point says of itself: the word its desc goes by in the messages, the knob of its phases, whether its workspace holds shells and the
	// segments it holds the variable call's parts for (0: none), whether it writes blob rows, whether its workspace holds the
	// search's parts and whether the search takes every level; and the error metric its decisions are taken by (an aclhip_error_metric: the entry points without one say
	// ACLHIP_METRIC_QVVF); and whether it takes an additive base, and the caller's (the _additive entry points: it may be null, which
	// the check refuses). The rest of what tells the raw and the drop-w call apart is in the desc: the formats and the shell metadata, 0
	// for the raw call.
	struct transform_compress_kind
	{
		const char* name; const char* phases_knob; bool with_shells; uint32_t max_segments = 0; bool with_rows = true; bool with_search = false; bool with_levels = false; uint32_t metric = ACLHIP_METRIC_QVVF;
		bool with_base = false; const aclhip_additive_base* base = nullptr;
		transform_compress_kind with_metric(uint32_t error_metric) const { transform_compress_kind kind = *this; kind.metric = error_metric; return kind; }
		transform_compress_kind with_additive_base(const aclhip_additive_base* additive_base) const { transform_compress_kind kind = *this; kind.with_base = true; kind.base = additive_base; return kind; }
		// the format its kernels apply: ACLHIP_ADDITIVE_NONE for every call without a base (only behind the check)
		uint32_t additive_format() const { return with_base && base != nullptr ? base->additive_format : uint32_t(ACLHIP_ADDITIVE_NONE); }
	};

	// the segments of the longest array a caller announces (a desc of 0 max_samples is refused: it counts as 1 here)
	uint32_t variable_max_segments_of(uint32_t max_samples) { return variable_split_of(std::max(max_samples, 1u)).num_segments; }

	const transform_compress_kind k_transform_compress_kind = { "transform compress", "ACLHIP_TRANSFORM_COMPRESS_PHASES", false };
	const transform_compress_kind k_tracks_compress_kind = { "tracks compress", "ACLHIP_TRACKS_COMPRESS_PHASES", true };
	transform_compress_kind variable_compress_kind_of(uint32_t max_samples) { return { "variable compress", "ACLHIP_VARIABLE_COMPRESS_PHASES", true, variable_max_segments_of(max_samples) }; }
	transform_compress_kind bit_rate_search_kind_of(uint32_t max_samples) { return { "bit rate search", "ACLHIP_FIND_BIT_RATES_PHASES", true, variable_max_segments_of(max_samples), false, true }; }
	transform_compress_kind bit_rate_level_search_kind_of(uint32_t max_samples) { return { "bit rate level search", "ACLHIP_FIND_BIT_RATES_LEVEL_PHASES", true, variable_max_segments_of(max_samples), false, true, true }; }

	// The workspace: where each part begins and where the last one ends, each part rounded up to 16 bytes (128 bits wide: see
	// aclhip_scalar_compress_workspace_bytes). The raw call has the first three parts, aclhip_compress_tracks_batch the shells
	// ({ local shell distance, precision } per instance and track) behind them, aclhip_compress_tracks_variable_batch behind those the
	// clip ranges (18 floats per instance and track) and, per instance and segment of max_samples (max_segments; 0: none of the three),
	// a variable_segment and the prefix sums (a dword per sub-track); aclhip_find_bit_rates_batch behind those, per instance and segment,
	// a search_segment and, per track, the segment range (18 floats), the segment's shell and an entry of the chain under work;
	// aclhip_find_bit_rates_level_batch behind those, per instance, segment and track, the memo of its object phase (three dwords: what
	// increasing that link of the chain by 1, 2 and 3 gives in this round). The size functions and the launch record both read it.
	struct transform_workspace_layout
	{
		unsigned __int128 instances = 0, track_flags, animated, shells, clip_ranges, segments, prefix, search_segments, segment_ranges, segment_shells, chains, memo, total;
		transform_workspace_layout(uint32_t num_instances, uint32_t max_tracks, const transform_compress_kind& kind)
		{
			const auto part = [](unsigned __int128 bytes) { return (bytes + 15u) & ~(unsigned __int128)15; };
			const unsigned __int128 n = num_instances, max_segments = kind.max_segments;
			track_flags = instances + part(n * sizeof(compress_instance));
			animated = track_flags + part(n * max_tracks);
			shells = animated + part(n * max_tracks * 3u * sizeof(uint16_t));
			clip_ranges = shells + (kind.with_shells ? part(n * max_tracks * sizeof(float2)) : 0);
			segments = clip_ranges + (max_segments != 0 ? part(n * max_tracks * k_variable_range_floats * sizeof(float)) : 0);
			prefix = segments + part(n * max_segments * sizeof(variable_segment));
			search_segments = prefix + part(n * max_segments * max_tracks * 3u * sizeof(uint32_t));
			segment_ranges = search_segments + (kind.with_search ? part(n * max_segments * sizeof(search_segment)) : 0);
			segment_shells = segment_ranges + (kind.with_search ? part(n * max_segments * max_tracks * k_search_segment_floats * sizeof(float)) : 0);
			chains = segment_shells + (kind.with_search ? part(n * max_segments * max_tracks * sizeof(float2)) : 0);
			memo = chains + (kind.with_search ? part(n * max_segments * max_tracks * sizeof(uint16_t)) : 0);
			total = memo + (kind.with_levels ? part(n * max_segments * max_tracks * 3u * sizeof(uint32_t)) : 0);
		}
	};
	uint64_t transform_workspace_bytes(uint32_t num_instances, uint32_t max_tracks, const transform_compress_kind& kind)
	{
		return compress_size_of(transform_workspace_layout(num_instances, max_tracks, kind).total);
	}
}

extern "C" uint64_t aclhip_transform_compress_bound(uint32_t num_tracks, uint32_t num_samples, uint32_t flags)
{
	// headers, 2 bits per sub-track in words of 16, every sub-track animated (a constant one takes its 16 or 12 bytes once, and an array
	// has a sample), metadata or the tail
	const unsigned __int128 tracks = num_tracks;
	unsigned __int128 bytes = k_transform_blob_headers + 12u * ((tracks + 15u) / 16u) + 40u * tracks * num_samples;
	if ((flags & (ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES | ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS)) != 0)
		bytes += 4u * tracks + ((flags & ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS) != 0 ? 48u * tracks : 0u) + sizeof(optional_metadata_header);
	else
		bytes += 15u;
	return compress_size_of(bytes);
}

extern "C" uint64_t aclhip_transform_compress_workspace_bytes(uint32_t num_instances, uint32_t max_tracks)
{
	return transform_workspace_bytes(num_instances, max_tracks, k_transform_compress_kind);
}

extern "C" uint64_t aclhip_compress_tracks_workspace_bytes(uint32_t num_instances, uint32_t max_tracks)
{
	return transform_workspace_bytes(num_instances, max_tracks, k_tracks_compress_kind);
}

extern "C" uint32_t aclhip_variable_compress_num_segments(uint32_t num_samples)
{
	return variable_split_of(num_samples).num_segments;
}

extern "C" uint64_t aclhip_variable_compress_bound(uint32_t num_tracks, uint32_t num_samples, uint32_t flags)
{
	// every sub-track animated at rate 24: headers, start indices, segment headers, types, 24 bytes of clip range per sub-track; per
	// segment a format byte per sub-track (rotations padded to 4), the byte to an even offset, 6 range bytes per padded sub-track, up
	// to 3 bytes to the stream; 36 bytes per track and sample; up to 3 bytes to the metadata, or the tail
	const unsigned __int128 tracks = num_tracks, segments = variable_split_of(num_samples).num_segments;
	const unsigned __int128 num_variable = ((tracks + 3u) & ~(unsigned __int128)3) + 2u * tracks;
	unsigned __int128 bytes = k_transform_header_offset + k_segment_start_indices_offset + (segments > 1 ? 4u * (segments + 1u) : 0u) + 16u * segments
		+ 12u * ((tracks + 15u) / 16u) + 72u * tracks + segments * (num_variable + 1u + (segments > 1 ? 6u * num_variable : 0u) + 3u) + 36u * tracks * num_samples;
	if ((flags & (ACLHIP_COMPRESS_INCLUDE_PARENT_TRACK_INDICES | ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS)) != 0)
		bytes += 3u + 4u * tracks + ((flags & ACLHIP_COMPRESS_INCLUDE_TRACK_DESCRIPTIONS) != 0 ? 48u * tracks : 0u) + sizeof(optional_metadata_header);
	else
		bytes += 15u;
	return compress_size_of(bytes);
}

extern "C" uint64_t aclhip_compress_variable_workspace_bytes(uint32_t num_instances, uint32_t max_tracks, uint32_t max_samples)
{
	return transform_workspace_bytes(num_instances, max_tracks, variable_compress_kind_of(max_samples));
}

extern "C" uint64_t aclhip_find_bit_rates_workspace_bytes(uint32_t num_instances, uint32_t max_tracks, uint32_t max_samples)
{
	return transform_workspace_bytes(num_instances, max_tracks, bit_rate_search_kind_of(max_samples));
}

extern "C" uint64_t aclhip_find_bit_rates_level_workspace_bytes(uint32_t num_instances, uint32_t max_tracks, uint32_t max_samples)
{
	return transform_workspace_bytes(num_instances, max_tracks, bit_rate_level_search_kind_of(max_samples));
}

namespace
{
	// The kernels between the shell and the hash, per rotation format: quatf_full (the raw call's: no metric enters it), quatf_drop_w_full
	// per error metric
	struct transform_compress_kernels { void (*analyze)(transform_compress_launch), (*layout)(transform_compress_launch), (*stream)(transform_compress_launch); };
	const transform_compress_kernels k_transform_compress_kernels[3] =
	{
		{ transform_compress_analyze_kernel, transform_compress_layout_kernel<false>, transform_compress_stream_kernel<false> },
		{ tracks_compress_analyze_kernel<k_metric_qvvf>, transform_compress_layout_kernel<true>, transform_compress_stream_kernel<true> },
		{ tracks_compress_analyze_kernel<k_metric_matrix>, transform_compress_layout_kernel<true>, transform_compress_stream_kernel<true> },
	};

	// The kernels that decide by the error metric, per metric: the shell (its vote) and the variable call's analysis, which the drop-w
	// call, the variable call and the search share, and the search's two phases, the object phase without and with the levels
	// -- and, for a call with an additive base of a format other than NONE, the seven kernels the base enters: those five, the drop-w
	// call's analysis and the search's segment kernel (S0), which no metric enters. The qvvf metric alone has them: the reference has
	// no additive matrix metric.
	struct metric_kernels
	{
		void (*shell)(transform_compress_launch); void (*variable_analyze)(variable_compress_launch);
		void (*search_local)(bit_rate_search_launch); void (*search_object)(bit_rate_search_launch); void (*search_object_levels)(bit_rate_search_levels_launch);
		void (*tracks_analyze)(transform_compress_launch); void (*search_segment)(bit_rate_search_launch);
	};
	const metric_kernels k_metric_kernels[2] =
	{
		{ tracks_compress_shell_kernel<k_metric_qvvf>, variable_compress_analyze_kernel<k_metric_qvvf>, bit_rate_search_local_kernel<k_metric_qvvf>,
			bit_rate_search_object_kernel<k_metric_qvvf>, bit_rate_search_object_kernel<k_metric_qvvf, true>, tracks_compress_analyze_kernel<k_metric_qvvf>, bit_rate_search_segment_kernel<false> },
		{ tracks_compress_shell_kernel<k_metric_matrix>, variable_compress_analyze_kernel<k_metric_matrix>, bit_rate_search_local_kernel<k_metric_matrix>,
			bit_rate_search_object_kernel<k_metric_matrix>, bit_rate_search_object_kernel<k_metric_matrix, true>, tracks_compress_analyze_kernel<k_metric_matrix>, bit_rate_search_segment_kernel<false> },
	};
	const metric_kernels k_additive_kernels =
	{
		tracks_compress_shell_kernel<k_metric_qvvf, true>, variable_compress_analyze_kernel<k_metric_qvvf, true>, bit_rate_search_local_kernel<k_metric_qvvf, true>,
		bit_rate_search_object_kernel<k_metric_qvvf, false, true>, bit_rate_search_object_kernel<k_metric_qvvf, true, true>, tracks_compress_analyze_kernel<k_metric_qvvf, true>,
		bit_rate_search_segment_kernel<true>,
	};
	const metric_kernels& deciding_kernels_of(const transform_compress_kind& kind)
	{
		return kind.additive_format() != ACLHIP_ADDITIVE_NONE ? k_additive_kernels : k_metric_kernels[kind.metric];
	}

	// A smaller desc as the drop-w call's, which the shared check and the launch record read: the rotation format the call stands for
	// (the raw call the full one; the variable call and the search quatf_drop_w_full, which passes the format clauses: they have no
	// formats to choose), its own reserved words with the others, and the shell metadata where it has one (the raw call: none).
	template<class desc_type>
	aclhip_compress_tracks_desc compress_tracks_desc_of(const desc_type& desc, uint32_t rotation_format, uint64_t reserved = 0)
	{
		aclhip_compress_tracks_desc as_tracks = {};
		as_tracks.rotation_format = rotation_format;
		as_tracks.flags = desc.flags;
		as_tracks.max_tracks = desc.max_tracks;
		as_tracks.num_table_tracks = desc.num_table_tracks;
		as_tracks.default_pose = desc.default_pose;
		as_tracks.parent_indices = desc.parent_indices;
		as_tracks.track_precisions = desc.track_precisions;
		as_tracks.track_shell_distances = desc.track_shell_distances;
		as_tracks.precision = desc.precision;
		as_tracks.shell_distance = desc.shell_distance;
		as_tracks.workspace = desc.workspace;
		if constexpr (!std::is_same_v<desc_type, aclhip_transform_compress_desc>)
			as_tracks.shell_metadata = desc.shell_metadata;
		as_tracks.reserved[0] = desc.reserved[0] | reserved;
		as_tracks.reserved[1] = desc.reserved[1];
		return as_tracks;
	}

	// one count (num_table_tracks) for every per-track table a desc names
	bool transform_compress_has_table(const aclhip_compress_tracks_desc& desc)
	{
		return desc.default_pose != nullptr || desc.parent_indices != nullptr || desc.track_precisions != nullptr || desc.track_shell_distances != nullptr;
	}

	// A bit rate table, { rotation, translation, scale, 0 } per (instance, segment, track): the variable call reads one (or none), the
	// search writes one. Its bytes: an instance stride for every instance but the last, a segment stride for every segment but the
	// last, and a row.
	struct bit_rate_table
	{
		const void* pointer;
		uint64_t instance_stride, segment_stride;
		uint32_t max_segments, max_tracks;
		byte_range range(uint32_t num_instances) const
		{
			const unsigned __int128 n = num_instances;
			return { "the bit rate table", pointer, pointer != nullptr ? (n - (n != 0 ? 1u : 0u)) * instance_stride + (unsigned __int128)(max_segments - 1u) * segment_stride + 4u * (unsigned __int128)max_tracks : 0 };
		}
	};
	aclhip_status check_bit_rate_table(aclhip_context* context, const bit_rate_table& table)
	{
		if ((reinterpret_cast<uintptr_t>(table.pointer) & 3u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the bit rate table must be 4 byte aligned");
		if (table.pointer != nullptr && ((table.instance_stride | table.segment_stride) & 3u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the strides of the bit rate table are multiples of 4");
		return ACLHIP_OK;
	}

	// What a call writes besides a table -- the blob rows (a call without rows: none), the results, the workspace, the shell metadata --
	// and what it reads, each in the order the overlap passes name them
	void transform_compress_written(const transform_compress_kind& kind, uint32_t num_instances, const aclhip_compress_tracks_desc& desc, const void* blobs, uint64_t blob_stride_bytes,
		const aclhip_compress_result* results, byte_range (&written)[4])
	{
		const unsigned __int128 n = num_instances;
		written[0] = { "the blob rows", blobs, n * blob_stride_bytes };
		written[1] = { "the compress results", results, n * sizeof(aclhip_compress_result) };
		written[2] = { "the workspace", desc.workspace, transform_workspace_bytes(num_instances, desc.max_tracks, kind) };
		written[3] = { "the shell metadata", desc.shell_metadata, desc.shell_metadata != nullptr ? n * desc.max_tracks * sizeof(float2) : 0 };
	}
	void transform_compress_read(const aclhip_raw_tracks* raws, uint32_t num_instances, const aclhip_compress_tracks_desc& desc, byte_range (&read)[5])
	{
		const unsigned __int128 n = num_instances, table = desc.num_table_tracks;
		read[0] = { "the raw track handles", raws, n * sizeof(aclhip_raw_tracks) };
		read[1] = { "the default pose", desc.default_pose, desc.default_pose != nullptr ? table * 48u : 0 };
		read[2] = { "the parent indices", desc.parent_indices, desc.parent_indices != nullptr ? table * sizeof(uint32_t) : 0 };
		read[3] = { "the track precisions", desc.track_precisions, desc.track_precisions != nullptr ? table * sizeof(float) : 0 };
		read[4] = { "the track shell distances", desc.track_shell_distances, desc.track_shell_distances != nullptr ? table * sizeof(float) : 0 };
	}

	// the handles of the bases a call reads: none without a base or with ACLHIP_ADDITIVE_NONE
	byte_range additive_base_range(const transform_compress_kind& kind, uint32_t num_instances)
	{
		const bool read = kind.additive_format() != ACLHIP_ADDITIVE_NONE;
		return { "the additive base handles", read ? kind.base->base_raws : nullptr, read ? (unsigned __int128)num_instances * sizeof(aclhip_raw_tracks) : 0 };
	}

	// What the launch checks of its arguments before any device call, its own between the parts every compressor checks
	// (host_scalar_compress.inl). The raw call's desc has no shell metadata and the full formats: those clauses pass.
	aclhip_status check_transform_compress(aclhip_context* context, const transform_compress_kind& kind, const aclhip_raw_tracks* raws, uint32_t num_instances,
		const aclhip_compress_tracks_desc* desc, const void* blobs, uint64_t blob_stride_bytes, const aclhip_compress_result* results)
	{
		// (a call without rows has none to be null or misaligned, and none that could overlap)
		if (!kind.with_rows)
		{
			blobs = nullptr;
			blob_stride_bytes = 0;
		}
		if (kind.metric > ACLHIP_METRIC_QVVF_MATRIX3X4F)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown error metric %u", kind.metric);
		if (kind.with_base)
		{
			if (kind.base == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null additive base");
			if (kind.base->additive_format > ACLHIP_ADDITIVE_ADDITIVE1)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "unknown additive format %u", kind.base->additive_format);
			if (kind.base->reserved_word != 0 || kind.base->reserved[0] != 0 || kind.base->reserved[1] != 0)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "reserved fields of the additive base are not 0");
			if (kind.base->additive_format != ACLHIP_ADDITIVE_NONE && kind.base->base_raws == nullptr)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "additive format %u without base_raws", kind.base->additive_format);
			if (kind.base->additive_format != ACLHIP_ADDITIVE_NONE && (reinterpret_cast<uintptr_t>(kind.base->base_raws) & 3u) != 0)
				return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "base_raws must be 4 byte aligned");
		}
		if (const aclhip_status status = check_compress_buffers(context, kind.name, "raw track", raws, desc, blobs, blob_stride_bytes, results, kind.with_rows); status != ACLHIP_OK)
			return status;
		if ((reinterpret_cast<uintptr_t>(desc->default_pose) & 15u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the default pose must be 16 byte aligned");
		if (((reinterpret_cast<uintptr_t>(desc->parent_indices) | reinterpret_cast<uintptr_t>(desc->track_precisions) | reinterpret_cast<uintptr_t>(desc->track_shell_distances)) & 3u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the track tables must be 4 byte aligned");
		if ((reinterpret_cast<uintptr_t>(desc->shell_metadata) & 7u) != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "the shell metadata must be 8 byte aligned");
		if (const aclhip_status status = check_compress_settings(context, kind.name, *desc, k_transform_compress_flags); status != ACLHIP_OK)
			return status;
		if (!std::isfinite(desc->shell_distance) || desc->shell_distance < 0.0f)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a shell distance of %g: it must be finite and not negative", double(desc->shell_distance));
		if (desc->rotation_format == k_rotation_quatf_drop_w_variable)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "rotation format quatf_drop_w_variable is not built");
		if (desc->rotation_format != k_rotation_quatf_full && desc->rotation_format != k_rotation_quatf_drop_w_full)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a rotation format of %u: 0 (quatf_full) or 2 (quatf_drop_w_full)", desc->rotation_format);
		if (desc->rotation_format == k_rotation_quatf_full && kind.additive_format() != ACLHIP_ADDITIVE_NONE)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "rotation format quatf_full takes no additive base: the raw settings decide nothing by a metric");
		if (desc->translation_format == 1 || desc->scale_format == 1)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "vector format vector3f_variable is not built");
		if (desc->translation_format != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a translation format of %u: 0 (vector3f_full)", desc->translation_format);
		if (desc->scale_format != 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a scale format of %u: 0 (vector3f_full)", desc->scale_format);
		if (transform_compress_has_table(*desc) && desc->num_table_tracks == 0)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a track table with a count of 0");
		byte_range written[4], ranges[8] = {};		// (ranges: three free places in front of what is read, for check_compress_ranges)
		transform_compress_written(kind, num_instances, *desc, blobs, blob_stride_bytes, results, written);
		transform_compress_read(raws, num_instances, *desc, reinterpret_cast<byte_range (&)[5]>(ranges[3]));
		if (const aclhip_status status = check_compress_ranges(context, kind.name, *desc, uint64_t(written[2].bytes), num_instances, blobs, blob_stride_bytes, results, ranges); status != ACLHIP_OK)
			return status;
		// the fourth output, in a pass of its own behind that one: it overlaps no other and nothing that is read
		if (const aclhip_status status = check_no_overlap(context, &written[3], 1, ranges, 8); status != ACLHIP_OK)
			return status;
		// the bases' handles, where a call reads them: they overlap nothing that is written
		const byte_range base_range = additive_base_range(kind, num_instances);
		return check_no_overlap(context, written, 4, &base_range, 1);
	}

	// The launch record of a checked call: the tables, the settings and where the workspace's parts lie
	transform_compress_launch transform_compress_launch_of(aclhip_context* context, const transform_compress_kind& kind, const aclhip_raw_tracks* raws, uint32_t num_instances,
		const aclhip_compress_tracks_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, const compress_launch_shape& shape, const transform_workspace_layout& layout)
	{
		uint8_t* workspace = static_cast<uint8_t*>(desc->workspace);
		transform_compress_launch launch = {};
		launch.arrays = context->raw_tracks.d_records;
		launch.num_arrays = ACLHIP_MAX_RAW_TRACKS;
		launch.num_instances = num_instances;
		launch.raws = raws;
		launch.default_pose = static_cast<const f32x4*>(desc->default_pose);
		launch.parent_indices = desc->parent_indices;
		launch.track_precisions = desc->track_precisions;
		launch.track_shell_distances = desc->track_shell_distances;
		launch.table_tracks = transform_compress_has_table(*desc) ? desc->num_table_tracks : 0xFFFFFFFFu;
		launch.flags = desc->flags;
		launch.precision = desc->precision;
		launch.shell_distance = desc->shell_distance;
		launch.max_tracks = desc->max_tracks;
		launch.instances = reinterpret_cast<compress_instance*>(workspace + uint64_t(layout.instances));
		launch.track_flags = workspace + uint64_t(layout.track_flags);
		launch.animated = reinterpret_cast<uint16_t*>(workspace + uint64_t(layout.animated));
		launch.shells = kind.with_shells ? reinterpret_cast<float2*>(workspace + uint64_t(layout.shells)) : nullptr;
		launch.shell_metadata = static_cast<float2*>(desc->shell_metadata);
		launch.blobs = static_cast<uint8_t*>(blobs);
		launch.blob_stride_bytes = blob_stride_bytes;
		launch.results = reinterpret_cast<uint2*>(results);
		launch.waves_per_instance = shape.waves_per_instance;
		launch.rejected_count = context->d_rejected;
		launch.additive_format = kind.additive_format();
		launch.base_raws = launch.additive_format != ACLHIP_ADDITIVE_NONE ? kind.base->base_raws : nullptr;
		return launch;
	}

	// and of the variable call and the search: that one, the segments and the variable call's three parts of the workspace. The rates
	// are the variable call's own.
	variable_compress_launch variable_compress_launch_of(aclhip_context* context, const transform_compress_kind& kind, const aclhip_raw_tracks* raws, uint32_t num_instances,
		const aclhip_compress_tracks_desc* desc, uint32_t max_samples, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, const compress_launch_shape& shape,
		const transform_workspace_layout& layout)
	{
		uint8_t* workspace = static_cast<uint8_t*>(desc->workspace);
		variable_compress_launch launch = {};
		launch.base = transform_compress_launch_of(context, kind, raws, num_instances, desc, blobs, blob_stride_bytes, results, shape, layout);
		launch.max_samples = max_samples;
		launch.max_segments = kind.max_segments;
		launch.clip_ranges = reinterpret_cast<float*>(workspace + uint64_t(layout.clip_ranges));
		launch.segments = reinterpret_cast<variable_segment*>(workspace + uint64_t(layout.segments));
		launch.prefix = reinterpret_cast<uint32_t*>(workspace + uint64_t(layout.prefix));
		return launch;
	}

	// the blocks of a wave per (instance, segment), the waves in turn where the grid would not hold them
	uint32_t compress_segment_blocks_of(uint32_t num_instances, uint32_t max_segments)
	{
		return uint32_t(std::min<uint64_t>((uint64_t(num_instances) * max_segments - 1) / k_compress_waves_per_block + 1, 1u << 20));
	}

	// The raw and the drop-w entry point behind their own words: the check, the launch record and the launches -- four for quatf_full
	// (the raw call's), the shell in front of them and its own analysis for quatf_drop_w_full.
	aclhip_status compress_transform_tracks(aclhip_context* context, const transform_compress_kind& kind, const aclhip_raw_tracks* raws, uint32_t num_instances,
		const aclhip_compress_tracks_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
	{
		const aclhip_status status = check_transform_compress(context, kind, raws, num_instances, desc, blobs, blob_stride_bytes, results);
		if (status != ACLHIP_OK)
			return status;
		return launch_compress(context, &aclhip_context::raw_tracks, num_instances, stream_handle, [&](hipStream_t stream) -> aclhip_status
		{
			const compress_launch_shape shape = compress_launch_shape_of(num_instances, desc->max_tracks, blob_stride_bytes, kind.phases_knob);
			const transform_workspace_layout layout(num_instances, desc->max_tracks, kind);
			const transform_compress_launch launch = transform_compress_launch_of(context, kind, raws, num_instances, desc, blobs, blob_stride_bytes, results, shape, layout);
			const compress_hash_launch hash_launch = { launch.instances, num_instances, launch.blobs, blob_stride_bytes };

			// (the phases knob counts the call's own launches: four for quatf_full, five for quatf_drop_w_full)
			const bool drop_w = desc->rotation_format == k_rotation_quatf_drop_w_full;
			const transform_compress_kernels& kernels = k_transform_compress_kernels[drop_w ? 1u + kind.metric : 0u];
			const metric_kernels& deciding = deciding_kernels_of(kind);
			const dim3 block(shape.block_size);
			const compress_phase phases[] =
			{
				{ deciding.shell, dim3(shape.instance_blocks), block, launch },
				{ drop_w ? deciding.tracks_analyze : kernels.analyze, shape.track_blocks, block, launch },
				{ kernels.layout, dim3(shape.instance_blocks), block, launch },
				{ kernels.stream, dim3(shape.stream_blocks), block, launch },
				{ compress_hash_kernel, dim3(num_instances), dim3(k_wave_size), hash_launch },
			};
			return launch_compress_phases(context, stream, shape.phases, phases + (drop_w ? 0 : 1), drop_w ? 5 : 4);
		});
	}
}

extern "C" aclhip_status aclhip_compress_raw_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_transform_compress_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	// its desc as the larger one: the full formats and no shell metadata
	const aclhip_compress_tracks_desc as_tracks = compress_tracks_desc_of(desc != nullptr ? *desc : aclhip_transform_compress_desc{}, k_rotation_quatf_full);
	return compress_transform_tracks(context, k_transform_compress_kind, raws, num_instances, desc != nullptr ? &as_tracks : nullptr, blobs, blob_stride_bytes, results, stream_handle);
}

// The three calls that decide by an error metric, with the metric as an argument; the entry points without one are these with
// ACLHIP_METRIC_QVVF.
extern "C" aclhip_status aclhip_compress_tracks_metric_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_compress_tracks_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, uint32_t metric, void* stream_handle)
{
	return compress_transform_tracks(context, k_tracks_compress_kind.with_metric(metric), raws, num_instances, desc, blobs, blob_stride_bytes, results, stream_handle);
}

extern "C" aclhip_status aclhip_compress_tracks_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_compress_tracks_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	return aclhip_compress_tracks_metric_batch(context, raws, num_instances, desc, blobs, blob_stride_bytes, results, ACLHIP_METRIC_QVVF, stream_handle);
}

extern "C" aclhip_status aclhip_compress_tracks_additive_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_compress_tracks_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, const aclhip_additive_base* additive_base, void* stream_handle)
{
	return compress_transform_tracks(context, k_tracks_compress_kind.with_additive_base(additive_base), raws, num_instances, desc, blobs, blob_stride_bytes, results, stream_handle);
}

// The variable call: the shared check over its desc as the drop-w one, its own checks behind it, and its six launches.
namespace
{
aclhip_status compress_variable_tracks(aclhip_context* context, const transform_compress_kind& kind, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_compress_variable_desc* desc_or_null, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	const aclhip_compress_variable_desc& desc = desc_or_null != nullptr ? *desc_or_null : aclhip_compress_variable_desc{};
	const aclhip_compress_tracks_desc as_tracks = compress_tracks_desc_of(desc, k_rotation_quatf_drop_w_full, desc.reserved_rate | desc.reserved_word);
	if (const aclhip_status status = check_transform_compress(context, kind, raws, num_instances, desc_or_null != nullptr ? &as_tracks : nullptr, blobs, blob_stride_bytes, results); status != ACLHIP_OK)
		return status;
	if (desc.max_samples == 0)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a variable compress desc of 0 max_samples");
	const bit_rate_table table = { desc.bit_rates, desc.bit_rate_instance_stride, desc.bit_rate_segment_stride, kind.max_segments, desc.max_tracks };
	if (const aclhip_status status = check_bit_rate_table(context, table); status != ACLHIP_OK)
		return status;
	if (desc.bit_rates == nullptr && (desc.rotation_bit_rate > k_variable_raw_rate || desc.translation_bit_rate > k_variable_raw_rate || desc.scale_bit_rate > k_variable_raw_rate))
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "uniform bit rates of %u, %u and %u: 0 to 24", desc.rotation_bit_rate, desc.translation_bit_rate, desc.scale_bit_rate);
	// (the table alone is new: the shared check has held what is written against each other and against the rest of what is read)
	byte_range written[4];
	transform_compress_written(kind, num_instances, as_tracks, blobs, blob_stride_bytes, results, written);
	const byte_range table_range = table.range(num_instances);
	if (const aclhip_status status = check_no_overlap(context, written, 4, &table_range, 1); status != ACLHIP_OK)
		return status;
	return launch_compress(context, &aclhip_context::raw_tracks, num_instances, stream_handle, [&](hipStream_t stream) -> aclhip_status
	{
		const compress_launch_shape shape = compress_launch_shape_of(num_instances, desc.max_tracks, blob_stride_bytes, kind.phases_knob);
		const transform_workspace_layout layout(num_instances, desc.max_tracks, kind);
		variable_compress_launch launch = variable_compress_launch_of(context, kind, raws, num_instances, &as_tracks, desc.max_samples, blobs, blob_stride_bytes, results, shape, layout);
		launch.bit_rates = desc.bit_rates;
		launch.bit_rate_instance_stride = desc.bit_rate_instance_stride;
		launch.bit_rate_segment_stride = desc.bit_rate_segment_stride;
		launch.uniform_rates = uint32_t(desc.rotation_bit_rate) | (uint32_t(desc.translation_bit_rate) << 8) | (uint32_t(desc.scale_bit_rate) << 16);
		const compress_hash_launch hash_launch = { launch.base.instances, num_instances, launch.base.blobs, blob_stride_bytes };

		const metric_kernels& deciding = deciding_kernels_of(kind);
		const dim3 block(shape.block_size);
		const compress_phase phases[] =
		{
			{ deciding.shell, dim3(shape.instance_blocks), block, launch.base },
			{ deciding.variable_analyze, shape.track_blocks, block, launch },
			{ variable_compress_layout_kernel, dim3(shape.instance_blocks), block, launch },
			{ variable_compress_ranges_kernel, dim3(compress_segment_blocks_of(num_instances, kind.max_segments)), block, launch },
			{ variable_compress_stream_kernel, dim3(shape.stream_blocks), block, launch },
			{ compress_hash_kernel, dim3(num_instances), dim3(k_wave_size), hash_launch },
		};
		return launch_compress_phases(context, stream, shape.phases, phases, 6);
	});
}
}

extern "C" aclhip_status aclhip_compress_tracks_variable_metric_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_compress_variable_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, uint32_t metric, void* stream_handle)
{
	return compress_variable_tracks(context, variable_compress_kind_of(desc != nullptr ? desc->max_samples : 0).with_metric(metric), raws, num_instances, desc, blobs, blob_stride_bytes,
		results, stream_handle);
}

extern "C" aclhip_status aclhip_compress_tracks_variable_additive_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_compress_variable_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, const aclhip_additive_base* additive_base, void* stream_handle)
{
	return compress_variable_tracks(context, variable_compress_kind_of(desc != nullptr ? desc->max_samples : 0).with_additive_base(additive_base), raws, num_instances, desc, blobs,
		blob_stride_bytes, results, stream_handle);
}

extern "C" aclhip_status aclhip_compress_tracks_variable_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_compress_variable_desc* desc, void* blobs, uint64_t blob_stride_bytes, aclhip_compress_result* results, void* stream_handle)
{
	return aclhip_compress_tracks_variable_metric_batch(context, raws, num_instances, desc, blobs, blob_stride_bytes, results, ACLHIP_METRIC_QVVF, stream_handle);
}

// The search, of either kind: the shared check over its desc as the drop-w one, like the variable call; no rows; the table on the
// written side. The kind with the levels takes every level, has its memo in the workspace, and launches the level per instance in
// front of its own object phase.
namespace
{
aclhip_status find_bit_rates(aclhip_context* context, const transform_compress_kind& kind, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_find_bit_rates_desc* desc_or_null, uint8_t* bit_rates, uint64_t instance_stride, uint64_t segment_stride, aclhip_compress_result* results, void* stream_handle)
{
	const aclhip_find_bit_rates_desc& desc = desc_or_null != nullptr ? *desc_or_null : aclhip_find_bit_rates_desc{};
	const aclhip_compress_tracks_desc as_tracks = compress_tracks_desc_of(desc, k_rotation_quatf_drop_w_full, desc.reserved_word);
	const uint32_t max_segments = kind.max_segments;
	if (const aclhip_status status = check_transform_compress(context, kind, raws, num_instances, desc_or_null != nullptr ? &as_tracks : nullptr, nullptr, 0, results); status != ACLHIP_OK)
		return status;
	if (desc.max_samples == 0)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a %s desc of 0 max_samples", kind.name);
	if (kind.with_levels)
	{
		if (desc.level > 4 && desc.level != ACLHIP_LEVEL_AUTOMATIC)
			return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a level of %u: 0 (lowest), 1 (low), 2 (medium), 3 (high), 4 (highest) or %u (automatic)", desc.level, ACLHIP_LEVEL_AUTOMATIC);
	}
	else if (desc.level == 3 || desc.level == 4)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "level %u (%s) is not built: 0 (lowest), 1 (low) and 2 (medium) are", desc.level, desc.level == 3 ? "high" : "highest");
	else if (desc.level > 4)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a level of %u: 0 (lowest), 1 (low) or 2 (medium)", desc.level);
	if (bit_rates == nullptr)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "null bit rate table");
	const bit_rate_table table = { bit_rates, instance_stride, segment_stride, max_segments, desc.max_tracks };
	if (const aclhip_status status = check_bit_rate_table(context, table); status != ACLHIP_OK)
		return status;
	if (segment_stride < 4ull * desc.max_tracks)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "a segment stride of %llu: a written row takes 4 * max_tracks = %llu bytes", (unsigned long long)segment_stride, 4ull * desc.max_tracks);
	if ((unsigned __int128)instance_stride < (unsigned __int128)max_segments * segment_stride)
		return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "an instance stride of %llu: the %u rows of an instance take %u segment strides", (unsigned long long)instance_stride, max_segments, max_segments);
	// (the table, in the rows' place, alone is new among what is written: the shared check has held the other three against each other
	// and against what is read)
	byte_range written[4], read[5];
	transform_compress_written(kind, num_instances, as_tracks, nullptr, 0, results, written);
	transform_compress_read(raws, num_instances, as_tracks, read);
	written[0] = table.range(num_instances);
	if (const aclhip_status status = check_no_overlap(context, written, 1, read, 5); status != ACLHIP_OK)
		return status;
	if (const aclhip_status status = check_no_overlap(context, written, 4, nullptr, 0); status != ACLHIP_OK)
		return status;
	const byte_range base_range = additive_base_range(kind, num_instances);
	if (const aclhip_status status = check_no_overlap(context, written, 1, &base_range, 1); status != ACLHIP_OK)
		return status;
	return launch_compress(context, &aclhip_context::raw_tracks, num_instances, stream_handle, [&](hipStream_t stream) -> aclhip_status
	{
		const compress_launch_shape shape = compress_launch_shape_of(num_instances, desc.max_tracks, 16, kind.phases_knob);
		const transform_workspace_layout layout(num_instances, desc.max_tracks, kind);
		uint8_t* workspace = static_cast<uint8_t*>(desc.workspace);
		bit_rate_search_launch launch = {};
		launch.variable = variable_compress_launch_of(context, kind, raws, num_instances, &as_tracks, desc.max_samples, nullptr, 0, results, shape, layout);
		launch.table = bit_rates;
		launch.instance_stride = instance_stride;
		launch.segment_stride = segment_stride;
		launch.segments = reinterpret_cast<search_segment*>(workspace + uint64_t(layout.search_segments));
		launch.segment_ranges = reinterpret_cast<float*>(workspace + uint64_t(layout.segment_ranges));
		launch.segment_shells = reinterpret_cast<float2*>(workspace + uint64_t(layout.segment_shells));
		launch.chains = reinterpret_cast<uint16_t*>(workspace + uint64_t(layout.chains));
		const bit_rate_search_levels_launch levels_launch = { launch, reinterpret_cast<uint32_t*>(workspace + uint64_t(layout.memo)), desc.level };

		// a wave per (instance, segment), and for the local phase per (instance, segment, track), in turn where the grid would not hold them
		const uint32_t segment_blocks = compress_segment_blocks_of(num_instances, max_segments);
		const uint32_t track_blocks = uint32_t(std::min<unsigned __int128>((unsigned __int128)num_instances * max_segments * desc.max_tracks, 1u << 22));
		const dim3 block(shape.block_size);
		const metric_kernels& deciding = deciding_kernels_of(kind);
		const compress_phase phases[] =
		{
			{ deciding.shell, dim3(shape.instance_blocks), block, launch.variable.base },
			{ deciding.variable_analyze, shape.track_blocks, block, launch.variable },
			{ deciding.search_segment, dim3(segment_blocks), block, launch },
			{ deciding.search_local, dim3(track_blocks), dim3(k_wave_size), launch },
			{ deciding.search_object, dim3(segment_blocks), block, launch },
		};
		if (!kind.with_levels)
			return launch_compress_phases(context, stream, shape.phases, phases, 5);
		const compress_phase level_phases[] =
		{
			phases[0], phases[1], phases[2], phases[3],
			{ bit_rate_search_level_kernel, dim3(shape.instance_blocks), block, levels_launch },
			{ deciding.search_object_levels, dim3(segment_blocks), block, levels_launch },
		};
		return launch_compress_phases(context, stream, shape.phases, level_phases, 6);
	});
}
}

extern "C" aclhip_status aclhip_find_bit_rates_metric_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_find_bit_rates_desc* desc, uint8_t* bit_rates, uint64_t instance_stride, uint64_t segment_stride, aclhip_compress_result* results, uint32_t metric,
	void* stream_handle)
{
	return find_bit_rates(context, bit_rate_search_kind_of(desc != nullptr ? desc->max_samples : 0).with_metric(metric), raws, num_instances, desc, bit_rates, instance_stride, segment_stride,
		results, stream_handle);
}

extern "C" aclhip_status aclhip_find_bit_rates_level_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_find_bit_rates_desc* desc, uint8_t* bit_rates, uint64_t instance_stride, uint64_t segment_stride, aclhip_compress_result* results, uint32_t metric,
	void* stream_handle)
{
	return find_bit_rates(context, bit_rate_level_search_kind_of(desc != nullptr ? desc->max_samples : 0).with_metric(metric), raws, num_instances, desc, bit_rates, instance_stride, segment_stride,
		results, stream_handle);
}

extern "C" aclhip_status aclhip_find_bit_rates_additive_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_find_bit_rates_desc* desc, uint8_t* bit_rates, uint64_t instance_stride, uint64_t segment_stride, aclhip_compress_result* results,
	const aclhip_additive_base* additive_base, void* stream_handle)
{
	return find_bit_rates(context, bit_rate_level_search_kind_of(desc != nullptr ? desc->max_samples : 0).with_additive_base(additive_base), raws, num_instances, desc, bit_rates,
		instance_stride, segment_stride, results, stream_handle);
}

extern "C" aclhip_status aclhip_find_bit_rates_batch(aclhip_context* context, const aclhip_raw_tracks* raws, uint32_t num_instances,
	const aclhip_find_bit_rates_desc* desc, uint8_t* bit_rates, uint64_t instance_stride, uint64_t segment_stride, aclhip_compress_result* results, void* stream_handle)
{
	return aclhip_find_bit_rates_metric_batch(context, raws, num_instances, desc, bit_rates, instance_stride, segment_stride, results, ACLHIP_METRIC_QVVF, stream_handle);
}
