// host_ranges.inl -- part of aclhip.hip (one translation unit; included there in front of host_pose_buffers.inl, not compiled on its own).
// Host side: what the argument checks and the launches of the caller-buffer entry points share -- do two ranges of bytes overlap, does any
// output of a launch overlap what it reads or another output, and how many waves share an instance. (What only the launches over a
// caller's pose rows share -- the other clauses of their checks, their shape and their front -- stands at the top of host_pose_buffers.inl.)

namespace
{
	// do [a, a + a_stride * n) and [b, b + b_stride * n) share a byte? (a product past 2^64 ends at the top of the address space; an
	// empty range is a point: it lies inside a range that holds it strictly)
	bool pose_ranges_overlap(const void* a, uint64_t a_stride, const void* b, uint64_t b_stride, uint32_t num_instances)
	{
		const auto end_of = [&](const void* pointer, uint64_t stride)
		{
			const unsigned __int128 end = (unsigned __int128)reinterpret_cast<uintptr_t>(pointer) + (unsigned __int128)stride * num_instances;
			return end > (unsigned __int128)UINT64_MAX ? UINT64_MAX : uint64_t(end);
		};
		const uint64_t a_begin = reinterpret_cast<uintptr_t>(a), b_begin = reinterpret_cast<uintptr_t>(b);
		return a_begin < end_of(b, b_stride) && b_begin < end_of(a, a_stride);
	}

	// The same question of two ranges given by their sizes, in two forms: byte_ranges_meet takes an empty range as a point, as
	// pose_ranges_overlap does; to byte_ranges_overlap an empty range shares no byte. (an end past 2^64 is the top of the address space)
	bool byte_ranges_meet(const void* a, unsigned __int128 a_bytes, const void* b, unsigned __int128 b_bytes)
	{
		const unsigned __int128 a_begin = reinterpret_cast<uintptr_t>(a), b_begin = reinterpret_cast<uintptr_t>(b);
		return a_begin < b_begin + b_bytes && b_begin < a_begin + a_bytes;
	}
	bool byte_ranges_overlap(const void* a, unsigned __int128 a_bytes, const void* b, unsigned __int128 b_bytes)
	{
		return a_bytes != 0 && b_bytes != 0 && byte_ranges_meet(a, a_bytes, b, b_bytes);
	}

	// What is written overlaps nothing that is read and no other output; the inputs are only read and may share bytes. The first pair that
	// does: for each output in turn, every input, then every later output.
	struct byte_range { const char* name; const void* pointer; unsigned __int128 bytes; };
	aclhip_status check_no_overlap(const aclhip_context* context, const byte_range* outputs, size_t num_outputs, const byte_range* inputs, size_t num_inputs)
	{
		for (const byte_range* output = outputs; output != outputs + num_outputs; ++output)
		{
			for (const byte_range* input = inputs; input != inputs + num_inputs; ++input)
				if (byte_ranges_overlap(output->pointer, output->bytes, input->pointer, input->bytes))
					return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s overlap %s", output->name, input->name);
			for (const byte_range* other = output + 1; other != outputs + num_outputs; ++other)
				if (byte_ranges_overlap(output->pointer, output->bytes, other->pointer, other->bytes))
					return fail(context, ACLHIP_ERROR_INVALID_ARGUMENT, "%s overlap %s", output->name, other->name);
		}
		return ACLHIP_OK;
	}
	aclhip_status check_no_overlap(const aclhip_context* context, std::initializer_list<byte_range> outputs, std::initializer_list<byte_range> inputs)
	{
		return check_no_overlap(context, outputs.begin(), outputs.size(), inputs.begin(), inputs.size());
	}

	// The waves that share an instance's `units` (quads, floats or dwords of a row), units_per_wave to each and one at least. The wave
	// index of the kernels is 32 bits wide: a batch too large for a wave per share gets fewer, and its waves loop.
	uint32_t waves_per_instance_of(uint64_t units, uint64_t units_per_wave, uint32_t num_instances)
	{
		const uint64_t waves = std::max<uint64_t>((units + units_per_wave - 1) / units_per_wave, 1);
		return uint32_t(std::min<uint64_t>(waves, std::max<uint64_t>(0xFFFFFFF0ull / num_instances, 1)));
	}
}
